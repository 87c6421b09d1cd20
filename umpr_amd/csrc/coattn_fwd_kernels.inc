// The forward kernels of coattn.hip, compiled twice by it: COATTN_MASKED 0 gives coattn_scores_kernel, coattn_scores_bf16_kernel
// and coattn_finish_kernel - token for token the kernels from before the padding mask existed, so that they compile to the same
// code - and COATTN_MASKED 1 gives their *_masked_kernel forms with the validity bytes.  (A template switch shared by both was
// tried first: inlining the common body changed register allocation and scheduling of the unmasked kernels.)
#if COATTN_MASKED
#define COATTN_KERNEL(name) name##_masked_kernel
#define COATTN_MASK_PARAMS , const uint8_t* vu, const uint8_t* vi
#define COATTN_PAIR_VALID(r, j) (kuse && (rmask >> (r) & 1))
#else
#define COATTN_KERNEL(name) name##_kernel
#define COATTN_MASK_PARAMS
#define COATTN_PAIR_VALID(r, j) (kvalid && (j) < SL)
#endif

// One workgroup = 64 rows (j) x the column tiles of its split.  Wave (wi, wu) owns a 32 x 32 tile; lane half kh takes
// the reduction columns c = 64 kh + kk (any split of the 128 columns works as long as A and B agree), so a lane's 64
// operand values per matrix are contiguous: 16 ds_read_b128 each, all in registers before the 64 MFMAs, which run as
// two independent accumulator chains.
// MASKED: vu / vi are the validity bytes [B][SL] of the columns (user positions) and rows (item positions).  The 64 row bytes
// of the workgroup and the 64 column bytes of each tile go through LDS once (128 byte loads per tile); a lane keeps its 16
// rows' validity as one bit mask, so the predicate costs one register and no operand register is touched.
__global__ __launch_bounds__(256) void COATTN_KERNEL(coattn_scores)(ScoreParams p COATTN_MASK_PARAMS) {
  __shared__ __attribute__((aligned(16))) float Ts[64 * LDR];
  __shared__ __attribute__((aligned(16))) float Us[64 * LDR];
  __shared__ float xv[2][64]; __shared__ int xi[2][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wu = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  const int b = blockIdx.y, blk = blockIdx.x;
  const int SL = p.SL;
  const int j0 = blk * 64;
  const float* Tb = p.T + (long)b * SL * D;
  const float* Ub = p.Gu + (long)b * SL * D;

#if COATTN_MASKED
  __shared__ unsigned char vrow[64], vcol[64];
  if (tid < 64) vrow[tid] = j0 + tid < SL ? vi[(long)b * SL + j0 + tid] : 0;
#endif
  stage_tile_f32(Tb, j0, SL, Ts, tid);
  float rbest[16]; int ridx[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { rbest[r] = -INFINITY; ridx[r] = 0x7fffffff; }
  __syncthreads();
#if COATTN_MASKED
  unsigned rmask = 0;   // bit r: row mfma_row(r, lane) of this wave is inside SL and valid
#pragma unroll
  for (int r = 0; r < 16; ++r) rmask |= (vrow[wi * 32 + mfma_row(r, lane)] ? 1u : 0u) << r;
#endif
  float4 ta[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) ta[q] = *reinterpret_cast<const float4*>(Ts + (wi * 32 + l31) * LDR + 64 * kh + 4 * q);

  const int ntile = (SL + 63) / 64;
  const int tper = (ntile + p.ksplit - 1) / p.ksplit;
  const int ut_end = min(ntile, ((int)blockIdx.z + 1) * tper);
  for (int ut = blockIdx.z * tper; ut < ut_end; ++ut) {
    const int k0 = ut * 64;
    __syncthreads();
#if COATTN_MASKED
    if (tid < 64) vcol[tid] = k0 + tid < SL ? vu[(long)b * SL + k0 + tid] : 0;
#endif
    stage_tile_f32(Ub, k0, SL, Us, tid);
    __syncthreads();
    float4 ub[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) ub[q] = *reinterpret_cast<const float4*>(Us + (wu * 32 + l31) * LDR + 64 * kh + 4 * q);
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      acc0 = mfma32(ta[q].x, ub[q].x, acc0);
      acc1 = mfma32(ta[q].y, ub[q].y, acc1);
      acc0 = mfma32(ta[q].z, ub[q].z, acc0);
      acc1 = mfma32(ta[q].w, ub[q].w, acc1);
    }
    const int kcol = k0 + wu * 32 + l31;
    const bool kvalid = kcol < SL;
#if COATTN_MASKED
    const bool kuse = vcol[wu * 32 + l31] != 0;   // the column takes part in maxima (it is written either way)
#endif
    float cbest = -INFINITY; int cidx = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = j0 + wi * 32 + mfma_row(r, lane);
      const float a = tanhf(acc0[r] + acc1[r]);
      if (COATTN_PAIR_VALID(r, j)) {
        better_first(rbest[r], ridx[r], a, kcol);
        better_first(cbest, cidx, a, j);
      }
    }
    // column max: combine the two lane halves (rows +4), then the two wi waves
    {
      const float ov = __shfl_xor(cbest, 32, 64);
      const int oi = __shfl_xor(cidx, 32, 64);
      better_first(cbest, cidx, ov, oi);
    }
    if (wi == 1 && kh == 0) { xv[wu][l31] = cbest; xi[wu][l31] = cidx; }
    __syncthreads();
    if (wi == 0 && kh == 0) {
      better_first(cbest, cidx, xv[wu][l31], xi[wu][l31]);
      if (kvalid) {
        const long o = ((long)b * p.nblk + blk) * SL + kcol;
        p.colmax_part[o] = cbest;
        p.argcol_part[o] = cidx;
      }
    }
  }
  // row max: reduce over the 32 lanes of each half (columns), then over the two wu waves
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = rbest[r]; int i = ridx[r];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(i, o, 64);
      better_first(v, i, ov, oi);
    }
    rbest[r] = v; ridx[r] = i;
  }
  // rows of this wave: wi*32 + mfma_row(r, lane); lanes l31==0 of each half hold the result
  if (wu == 1 && l31 == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jr = wi * 32 + mfma_row(r, lane);
      xv[0][jr] = rbest[r]; xi[0][jr] = ridx[r];
    }
  }
  __syncthreads();
  if (wu == 0 && l31 == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jr = wi * 32 + mfma_row(r, lane);
      float v = rbest[r]; int i = ridx[r];
      better_first(v, i, xv[0][jr], xi[0][jr]);
      if (j0 + jr < SL) {
        const long o = ((long)b * p.ksplit + blockIdx.z) * SL + j0 + jr;
        p.rowmax_part[o] = v;
        p.argrow_part[o] = i;
      }
    }
  }
}

// The same tile loop with the score contraction on v_mfma_f32_32x32x16_bf16 (BASELINE.json configs[4]: "MFMA bf16 ...
// attention"): T and G_u rows are rounded to bf16 when they are staged, products accumulate in fp32, tanh / max /
// argmax stay fp32.  LDS rows of 128 bf16 are padded to 136 (272 B = 17 slots of 16 B): conflict-free ds_read_b128.
__global__ __launch_bounds__(256) void COATTN_KERNEL(coattn_scores_bf16)(ScoreParams p COATTN_MASK_PARAMS) {
  constexpr int LDB = 136;
  __shared__ __attribute__((aligned(16))) __bf16 Ts[64 * LDB];
  __shared__ __attribute__((aligned(16))) __bf16 Us[64 * LDB];
  __shared__ float xv[2][64]; __shared__ int xi[2][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wu = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  const int b = blockIdx.y, blk = blockIdx.x;
  const int SL = p.SL;
  const int j0 = blk * 64;
  const float* Tb = p.T + (long)b * SL * D;
  const float* Ub = p.Gu + (long)b * SL * D;
  auto stage = [&](const float* src, int row0, __bf16* dst) {
    float4 v[8];                                        // every load in flight before the first use (clamped rows)
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
      const bool ok = row0 + j < SL;
      bf16x4_t o;
      o[0] = (__bf16)(ok ? v[i].x : 0.f); o[1] = (__bf16)(ok ? v[i].y : 0.f);
      o[2] = (__bf16)(ok ? v[i].z : 0.f); o[3] = (__bf16)(ok ? v[i].w : 0.f);
      *reinterpret_cast<bf16x4_t*>(dst + j * LDB + c4) = o;
    }
  };
  stage(Tb, j0, Ts);
  float rbest[16]; int ridx[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { rbest[r] = -INFINITY; ridx[r] = 0x7fffffff; }
#if COATTN_MASKED
  __shared__ unsigned char vrow[64], vcol[64];
  if (tid < 64) vrow[tid] = j0 + tid < SL ? vi[(long)b * SL + j0 + tid] : 0;
  __syncthreads();
  unsigned rmask = 0;   // as in the fp32 kernel
#pragma unroll
  for (int r = 0; r < 16; ++r) rmask |= (vrow[wi * 32 + mfma_row(r, lane)] ? 1u : 0u) << r;
#endif
  const int ntile = (SL + 63) / 64;
  const int tper = (ntile + p.ksplit - 1) / p.ksplit;
  const int ut_end = min(ntile, ((int)blockIdx.z + 1) * tper);
  for (int ut = blockIdx.z * tper; ut < ut_end; ++ut) {
    const int k0 = ut * 64;
    __syncthreads();
#if COATTN_MASKED
    if (tid < 64) vcol[tid] = k0 + tid < SL ? vu[(long)b * SL + k0 + tid] : 0;
#endif
    stage(Ub, k0, Us);
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(Ts + (wi * 32 + l31) * LDB + ks * 16 + 8 * kh);
      const bf16x8_t u = *reinterpret_cast<const bf16x8_t*>(Us + (wu * 32 + l31) * LDB + ks * 16 + 8 * kh);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, u, acc, 0, 0, 0);
    }
    const int kcol = k0 + wu * 32 + l31;
    const bool kvalid = kcol < SL;
#if COATTN_MASKED
    const bool kuse = vcol[wu * 32 + l31] != 0;
#endif
    float cbest = -INFINITY; int cidx = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = j0 + wi * 32 + mfma_row(r, lane);
      const float a = tanhf(acc[r]);
      if (COATTN_PAIR_VALID(r, j)) {
        better_first(rbest[r], ridx[r], a, kcol);
        better_first(cbest, cidx, a, j);
      }
    }
    {
      const float ov = __shfl_xor(cbest, 32, 64);
      const int oi = __shfl_xor(cidx, 32, 64);
      better_first(cbest, cidx, ov, oi);
    }
    if (wi == 1 && kh == 0) { xv[wu][l31] = cbest; xi[wu][l31] = cidx; }
    __syncthreads();
    if (wi == 0 && kh == 0) {
      better_first(cbest, cidx, xv[wu][l31], xi[wu][l31]);
      if (kvalid) {
        const long o = ((long)b * p.nblk + blk) * SL + kcol;
        p.colmax_part[o] = cbest;
        p.argcol_part[o] = cidx;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = rbest[r]; int i = ridx[r];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(i, o, 64);
      better_first(v, i, ov, oi);
    }
    rbest[r] = v; ridx[r] = i;
  }
  if (wu == 1 && l31 == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jr = wi * 32 + mfma_row(r, lane);
      xv[0][jr] = rbest[r]; xi[0][jr] = ridx[r];
    }
  }
  __syncthreads();
  if (wu == 0 && l31 == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jr = wi * 32 + mfma_row(r, lane);
      float v = rbest[r]; int i = ridx[r];
      better_first(v, i, xv[0][jr], xi[0][jr]);
      if (j0 + jr < SL) {
        const long o = ((long)b * p.ksplit + blockIdx.z) * SL + j0 + jr;
        p.rowmax_part[o] = v;
        p.argrow_part[o] = i;
      }
    }
  }
}



// 1024 threads per (sample, side): the weighted sums over the SL positions run as 8 chains of SL/8 terms per column.  Side 0 =
// the user's columns (colmax -> soft_u -> atte_u), side 1 = the item's rows; one workgroup each (grid (B, 2)): at batch 32 a grid
// of B workgroups doing both sides one after the other left 7/8 of the chip idle for 33 us.
// MASKED: a position whose merged index is still the initialiser had no valid partner or is masked itself - undefined.  It
// is saved as max = +0.0, arg = -1, soft = +0.0 and stays out of the softmax (its slot holds -inf, then 0); a side without any
// defined position has mx = -inf and z = 0, and neither enters an expf or a division.
__global__ __launch_bounds__(1024) void COATTN_KERNEL(coattn_finish)(FinishParams p) {
  extern __shared__ float sm[];  // s[SL]
  __shared__ float red[16];
  __shared__ float part[8][D];
  const int tid = threadIdx.x, b = blockIdx.x, side = blockIdx.y, SL = p.SL;
  const float* max_part = side ? p.rowmax_part : p.colmax_part;
  const int* arg_part = side ? p.argrow_part : p.argcol_part;
  const int nparts = side ? p.ksplit : p.nblk;     // (row parts: ascending column ranges, ties keep the first column)
  float* vmax = side ? p.rowmax : p.colmax;
  int* varg = side ? p.argrow : p.argcol;
  float* soft = side ? p.soft_i : p.soft_u;
  float* sv = sm;
  float mx = -INFINITY;
  for (int k = tid; k < SL; k += 1024) {
    float v = -INFINITY; int idx = 0x7fffffff;
    for (int q = 0; q < nparts; ++q) {
      const long o = ((long)b * nparts + q) * SL + k;
      better_first(v, idx, max_part[o], arg_part[o]);
    }
#if COATTN_MASKED
    const bool defined = idx != 0x7fffffff;
    vmax[(long)b * SL + k] = defined ? v : 0.f; varg[(long)b * SL + k] = defined ? idx : -1;
#else
    vmax[(long)b * SL + k] = v; varg[(long)b * SL + k] = idx;
#endif
    sv[k] = v; mx = fmaxf(mx, v);
  }
  mx = block_max(mx, red);
  float z = 0.f;
  for (int k = tid; k < SL; k += 1024) {
#if COATTN_MASKED
    const float e = sv[k] == -INFINITY ? 0.f : expf(sv[k] - mx);
#else
    const float e = expf(sv[k] - mx);
#endif
    sv[k] = e; z += e;
  }
  z = block_sum(z, red);
  for (int k = tid; k < SL; k += 1024) {
#if COATTN_MASKED
    sv[k] = z > 0.f ? sv[k] / z : 0.f;
#else
    sv[k] /= z;
#endif
    soft[(long)b * SL + k] = sv[k];
  }
  __syncthreads();
  const int c = tid & 127, grp = tid >> 7;
  const float* G = (side ? p.Gi : p.Gu) + (long)b * SL * D;
  float a = 0.f;
#pragma unroll 4
  for (int k = grp; k < SL; k += 8) a += sv[k] * G[(long)k * D + c];
  part[grp][c] = a;
  __syncthreads();
  if (grp == 0) {
    const float v = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) + ((part[4][c] + part[5][c]) + (part[6][c] + part[7][c]));
    if (side == 0) p.atte_u[(long)b * p.ld_u + c] = v; else p.atte_i[(long)b * p.ld_i + c] = v;
  }
}

#undef COATTN_KERNEL
#undef COATTN_MASK_PARAMS
#undef COATTN_PAIR_VALID
