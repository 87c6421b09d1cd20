// VGG16 3x3 / stride 1 / pad 1 convolution for gfx950 in exact fp32 (v_mfma_f32_32x32x2_f32), NCHW in and out.
//
//  forward / dgrad : implicit GEMM  D[cout][pixel] = sum_k Wm[cout][k] * im2col(x)[k][pixel],  k = c*9 + kh*3 + kw
//                    (torch's OIHW flatten, so the forward weight matrix is the parameter itself).  dgrad is the
//                    same kernel on the flip-transposed weights Wt[cin][cout*9+tap'] = W[cout][cin][8-tap'].
//                    MFMA-A = weights (rows = output channel), MFMA-B = pixels (lanes run along x), so loads of x and
//                    stores of y are 128-B row segments.  Epilogue: +bias, ReLU; or (dgrad) * [mask_src > 0].
//  wgrad           : per workgroup a 64(cout) x 64(cin) x 9(tap) tile, K = pixels; the gz tile and the x halo patch
//                    of a 32-pixel segment are staged once in LDS and serve all nine taps (9 accumulator tiles per
//                    wave).  Split-K over pixel segments into slabs [split][tap][cout][cin] + deterministic reduce.
//  dispatch        : umpr_conv3x3_plan (below, with the table of layer class x pass x mode) decides once per call between the
//                    first-layer kernels, the Winograd kernels of winograd.hip, the LDS-patch implicit GEMM and the generic
//                    gather kernel; umpr_conv3x3_run / umpr_conv3x3_wgrad launch what it names.
#include "umpr_common.h"
#include "umpr_internal.h"
#include "umpr_tiles.h"
#include <stdlib.h>
#include <type_traits>

namespace {

struct ConvParams {
  const float* x;     // [N][C][H][W]
  const float* wm;    // [Cout][C*9]
  const float* bias;  // [Cout] or null
  const float* mask;  // [N][Cout][H][W] or null: out *= (mask > 0)
  float* y;           // [N][Cout][H][W]
  int N, C, H, W, Cout, relu;
  long p0_base;  // first flat pixel of this launch (a layer may be covered by a main launch + a finer-tiled tail)
  long p_end;    // one past the last flat pixel of this launch
};

// Epilogue of the implicit-GEMM kernels: y = [mask > 0] relu?(tot + bias) for the TM x TN accumulator tiles of one wave.
// The first version tested p.bias / p.relu / p.mask and co < Cout per element, so each of a lane's 64 outputs was a chain of
// its own - branch, load bias[co], wait, add, 64-bit co * HW, branch, load mask[o], wait, select, store - and every load
// latency was exposed, 64 times in a row (gfx950 listing of <64,256,224>: 2800 instructions after the loop, 128 loads that each
// met an immediate s_waitcnt vmcnt(0)).  Here
//  * the pointer tests and "does this wave's tile end inside Cout" (TAIL) pick one instantiation, once per wave;
//  * the bias comes in once per accumulator row - 16 * TM loads in one batch - not once per column tile;
//  * the mask comes in batches of 16 * TM loads, one per column tile, and the batch of tile j + 1 is issued before the stores
//    of tile j, so one load latency is exposed per wave, not one per element;
//  * an element's offset is the per-lane base plus a compile-time multiple of HW;
//  * without TAIL the stores of a column tile sit under ONE exec mask (the lane has a pixel); with TAIL each is predicated.
// rowu = first output channel of the wave's tile (wave-uniform), half = lane >> 5, row0 = rowu + 4 * half = the lane's first
// channel; obase[j] = n * Cout * HW + yx of the lane's
// pixel in column tile j, or of ANY pixel of the launch when the lane has none (pv[j] false).
// Nothing outside the tensors is touched: a lane without a pixel loads the mask of the pixel obase names and stores nothing;
// rows co >= Cout load bias[Cout - 1] and the mask word of row Cout - 1 of that pixel and store nothing.
template <int TM, int TN, bool BIAS, bool MASK, bool TAIL>
__device__ __forceinline__ void igemm_epilogue_as(const f32x16 (&tot)[TM][TN], const ConvParams& p, int HW, int row0,
                                                  const long (&obase)[TN], const bool (&pv)[TN]) {
  const int Cout = p.Cout;
  const bool relu = p.relu != 0;
  float bv[TM][16];
  if constexpr (BIAS) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = row0 + i * 32 + mfma_row(r, 0);
        bv[i][r] = p.bias[TAIL ? min(co, Cout - 1) : co];
      }
  }
  float mv[2][TM][16];
  auto load_mask = [&](int j) {
    const float* mp = p.mask + obase[j] + (long)row0 * HW;
    const float* mlast = p.mask + obase[j] + (long)(Cout - 1) * HW;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ro = i * 32 + mfma_row(r, 0);
        mv[j & 1][i][r] = *(!TAIL || row0 + ro < Cout ? mp + (long)ro * HW : mlast);
      }
  };
  if constexpr (MASK) load_mask(0);
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    if constexpr (MASK) {
      if (j + 1 < TN) load_mask(j + 1);
    }
    if (pv[j]) {
      float* yp = p.y + obase[j] + (long)row0 * HW;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ro = i * 32 + mfma_row(r, 0);
          float v = tot[i][j][r];
          if constexpr (BIAS) v += bv[i][r];
          const float vr = fmaxf(v, 0.f);
          v = relu ? vr : v;
          if constexpr (MASK) v = mv[j & 1][i][r] > 0.f ? v : 0.f;
          if (!TAIL || row0 + ro < Cout) yp[(long)ro * HW] = v;
        }
    }
  }
}

template <int TM, int TN>
__device__ __forceinline__ void igemm_epilogue(const f32x16 (&tot)[TM][TN], const ConvParams& p, int HW, int rowu, int half,
                                               const long (&obase)[TN], const bool (&pv)[TN]) {
  const int row0 = rowu + 4 * half;
  auto run = [&](auto bias, auto mask) {
    if (rowu + TM * 32 <= p.Cout) igemm_epilogue_as<TM, TN, decltype(bias)::value, decltype(mask)::value, false>(tot, p, HW, row0, obase, pv);
    else igemm_epilogue_as<TM, TN, decltype(bias)::value, decltype(mask)::value, true>(tot, p, HW, row0, obase, pv);
  };
  using T = std::true_type;
  using F = std::false_type;
  if (p.mask) {
    if (p.bias) run(T{}, T{});
    else run(F{}, T{});
  } else {
    if (p.bias) run(T{}, F{});
    else run(F{}, F{});
  }
}

template <int BM, int BN>
__global__ __launch_bounds__(256) void conv3x3_igemm_kernel(ConvParams p) {
  using LA = TileRegs<BM, true>;
  constexpr int LDA = LA::LD;
  constexpr int LDB = BN;
  constexpr int WTM = BM / 2, WTN = BN / 2;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int KROWS = 256 / BN;       // k rows staged per pass
  constexpr int NPASS = BK / KROWS;     // scalar im2col loads per thread per stage
  __shared__ __attribute__((aligned(16))) float As[2][BK * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK * LDB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int HW = p.H * p.W;
  const long NP = p.p_end;
  const long p0 = p.p0_base + (long)blockIdx.x * BN;
  const int m0 = blockIdx.y * BM;
  const int K = p.C * 9;
  const int vecA = (K & 3) == 0;

  // this thread's im2col pixel (fixed for the whole K loop)
  const int pl = tid % BN, krow = tid / BN;
  const long pp = p0 + pl;
  const bool pvalid = pp < NP;
  int tapmask = 0;
  long xbase = 0;
  if (pvalid) {
    const int n = (int)(pp / HW), yx = (int)(pp % HW);
    const int y = yx / p.W, x = yx % p.W;
    xbase = (long)n * p.C * HW + yx;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
      if (yy >= 0 && yy < p.H && xx >= 0 && xx < p.W) tapmask |= 1 << t;
    }
  }

  // two-level accumulation: the MFMA chain runs over KFLUSH k-tiles, then folds into `tot`.  A single fp32 chain
  // over K = 4608 loses ~6x more bits than the blocked sums of the reference's CPU kernels (gradients through 13
  // conv layers showed it); chains of 128 restore parity at < 1% cost.
  f32x16 acc[TM][TN], tot[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; tot[i][j][r] = 0.f; }

  LA ra;
  float rb[NPASS];
  unsigned rbok = 0;
  auto load_b = [&](int k0) {
    rbok = 0;
#pragma unroll
    for (int j = 0; j < NPASS; ++j) {
      const int k = k0 + j * KROWS + krow;
      const int c = k / 9, t = k - c * 9;
      const bool ok = k < K && ((tapmask >> t) & 1);
      rb[j] = p.x[ok ? xbase + (long)c * HW + (t / 3 - 1) * p.W + (t % 3 - 1) : 0];  // branch-free, select at store
      rbok |= (unsigned)ok << j;
    }
  };
  auto store_b = [&](float* S) {
#pragma unroll
    for (int j = 0; j < NPASS; ++j) S[(j * KROWS + krow) * LDB + pl] = ((rbok >> j) & 1) ? rb[j] : 0.f;
  };

  const int nt = (K + BK - 1) / BK;
  ra.load(p.wm, K, nullptr, m0, p.Cout, 0, K, vecA, tid);
  load_b(0);
  ra.store(As[0], tid);
  store_b(Bs[0]);
  __syncthreads();
  const int l31 = lane & 31, kh = lane >> 5;
  // outer loop = one MFMA accumulation chain (KFLUSH stages): inside it the accumulators are written only by
  // MFMAs and stay in AGPRs (a conditional fold inside the stage loop made hipcc move all of them through VGPRs
  // every stage: 128 v_accvgpr moves + an MFMA pipeline drain per stage)
  for (int t0 = 0; t0 < nt; t0 += KFLUSH) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int t1 = min(nt, t0 + KFLUSH);
  for (int t = t0; t < t1; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) {
      ra.load(p.wm, K, nullptr, m0, p.Cout, (t + 1) * BK, K, vecA, tid);
      load_b((t + 1) * BK);
    }
    const float* as = As[cur] + wm * WTM + l31;
    const float* bs = Bs[cur] + wn * WTN + l31;
    float a[2][TM], b[2][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) a[0][i] = as[kh * LDA + i * 32];
#pragma unroll
    for (int j = 0; j < TN; ++j) b[0][j] = bs[kh * LDB + j * 32];
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      const int cb = kk & 1, nb = cb ^ 1;
      if (kk + 1 < BK / 2) {
#pragma unroll
        for (int i = 0; i < TM; ++i) a[nb][i] = as[(2 * (kk + 1) + kh) * LDA + i * 32];
#pragma unroll
        for (int j = 0; j < TN; ++j) b[nb][j] = bs[(2 * (kk + 1) + kh) * LDB + j * 32];
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch reads ahead of this step's MFMAs
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma32(a[cb][i], b[cb][j], acc[i][j]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (t + 1 < nt) {
      ra.store(As[cur ^ 1], tid);
      store_b(Bs[cur ^ 1]);
    }
    __syncthreads();
  }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) tot[i][j] += acc[i][j];
  }

  long obase[TN];
  bool pv[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const long pq = p0 + wn * WTN + j * 32 + l31;
    pv[j] = pq < NP;
    const long pc = pv[j] ? pq : p0;      // p0 < NP: the grid covers no tile past the end
    obase[j] = (pc / HW) * p.Cout * HW + pc % HW;
  }
  igemm_epilogue<TM, TN>(tot, p, HW, m0 + __builtin_amdgcn_readfirstlane(wm) * WTM, kh, obase, pv);
}

// ------------------------------------------------------------------------------------------------------------
// v2 of the implicit GEMM for the VGG map widths (W = H in {224,112,56,28,14}): instead of gathering an im2col
// tile element by element, each k-stage copies the raw input rows of CC = 4 channels that the 128-pixel tile
// touches (plus a one-pixel halo) into LDS with float4 loads, and the nine taps are formed when the MFMA-B
// fragment is read: lane address = per-lane pixel base + an immediate.  The inner loop has no VALU work at all
// (v1 spent 14 VALU instructions per MFMA on index arithmetic - rocprofv3 SQ_INSTS_VALU).
//  * "virtual rows": image n, row y lives at v = n*(H+2) + y + 1, so rows above/below an image are zero rows and a
//    tile of consecutive flat pixels may straddle two images.
//  * weights arrive PACKED (pack_weights_kernel): wp[m][stage][k'] with k' = 2*(c_lo*9 + tap) + half and channel
//    = 4*stage + c_lo + 2*half, zero-padded to whole stages.  The two k of one MFMA step then differ by a constant
//    LDS offset in the patch (2 planes), which goes into the per-lane base of the upper half-wave, and the weight
//    tile is staged with aligned float4 loads and compile-time LDS offsets.
//  * every global load is unconditional (clamped address; validity applied when the registers go to LDS) and the
//    stage body is branch-free; 2 waves/SIMD (launch bounds) let one workgroup's staging overlap the other's MFMAs.
constexpr int V2_CC = 4, V2_KC = V2_CC * 9;

// rows of the halo patch a BN-pixel tile can touch on a WxW map: rows spanned inside one image, +2 when a tile can
// straddle two images (virtual rows insert two zero rows between images), +2 halo
constexpr int v2_patch_rows(int W, int BN) {
  return ((BN - 1 + W - 1) / W + 1) + (((W * W) % BN) ? 2 : 0) + 2;
}

template <int BM, int BN, int W>
// three workgroups per CU for the 64-pixel tail tiles, except at 224x224 where the halo patch alone is 66 KB of LDS (two fit) and
// the staged rows take 176 registers - declaring 3 there only made hipcc report a missed occupancy target
__global__ __launch_bounds__(256, (BN == 64 && !(BM == 128 && W == 224) ? 3 : 2)) void conv3x3_igemm_v2_kernel(ConvParams p) {
  constexpr int PR = v2_patch_rows(W, BN);
  constexpr int CC = V2_CC, KC = V2_KC;
  // patch plane: pixel (row r, column x) lives at 4 + r * RW + x, RW = W + 4: every row starts on a 16-byte boundary, so a staged
  // float4 is ONE aligned ds_write_b128 (the first layout kept a left halo column at index 0: four scalar stores per float4 at a
  // stride of 4 floats - two-way bank conflicts on every one of them, a third of the kernel's LDS-active cycles,
  // profiles/r03_f_pmc_direct224_sq_counters.txt).  The zero slots W .. W+3 of a row serve as the right halo of that row and the
  // left halo of the next one; four leading zeros stand in front of row 0.
  constexpr int RW = W + 4, PLANE = PR * RW + 4;
  constexpr int LDA = BM + 2;
  constexpr int VEC = (W % 4 == 0) ? 4 : 2;
  constexpr int WV = W / VEC;
  constexpr int WTM = BM / 2, WTN = BN / 2;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int AU = BM * 9;                 // float4 units of one weight stage
  constexpr int AV = (AU + 255) / 256;
  constexpr int BU = CC * PR * WV;           // vector units of one patch stage
  constexpr int BV = (BU + 255) / 256;
  constexpr int SFLUSH = 4;                  // stages per MFMA accumulation chain (144 k)
  __shared__ __attribute__((aligned(16))) float As[2][KC * LDA];
  __shared__ __attribute__((aligned(16))) float Ps[2][CC * PLANE];
  __shared__ long rowsrc[PR];                // element offset of (n_r, c=0, yy, 0) or -1

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, half = lane >> 5;
  // square maps only (umpr_conv3x3_run requires H == W == the template W): the geometry is compile-time, so every split of a
  // flat pixel into image / row / column below is a multiply-shift, not a division sequence
  constexpr int H = W, HW = H * W, HP = H + 2;
  // XCD-aware tile order: workgroups b, b+8, b+16, ... share an XCD (and its L2).  The Cout/BM workgroups that read
  // the SAME pixel tile get consecutive slots on one XCD, so the input patch is fetched into that L2 once instead of
  // once per output-channel tile (FETCH_SIZE showed 2.6x the compulsory bytes with the pixel-major order).
  const int mt = (p.Cout + BM - 1) / BM;
  const int xcd = blockIdx.x & 7, qq = blockIdx.x >> 3;
  const long ptile = (long)(qq / mt) * 8 + xcd;
  const long NP = p.p_end;
  const long p0 = p.p0_base + ptile * BN;
  if (p0 >= NP) return;
  const int m0 = (qq % mt) * BM;
  const int ns = (p.C + CC - 1) / CC;
  const int Kp = ns * KC;
  const int n0 = (int)(p0 / HW);
  const int yx0 = (int)(p0 - (long)n0 * HW);  // the tile's first pixel inside image n0: pixel d of the tile is pixel yx0 + d
  const int y0 = yx0 / W;                     // counted from the start of image n0, so the per-lane arithmetic below is 32-bit

  // virtual row v_first - 1 + tid = n0 * HP + (y0 + tid): image n0 + t / HP, row t % HP - 1 with t = y0 + tid
  if (tid < PR) {
    const int t = y0 + tid;
    const int nr = n0 + t / HP;
    const int yy = t % HP - 1;
    rowsrc[tid] = (nr < p.N && yy >= 0 && yy < H) ? ((long)nr * p.C * H + yy) * W : -1;
  }
  // The staging writes columns 0 .. W-1 of all PR rows of all CC planes of a buffer in every stage (zeros where rowsrc is -1 or
  // the channel is past C), and both buffers are staged before their first fragment read.  What it never writes is the halo: the
  // four leading zeros of a plane and the slots W .. W+3 of each row, i.e. floats slot * RW .. slot * RW + 3 of a plane for slot
  // = 0 .. PR.  Only those are zeroed here, for good (the first version cleared both buffers whole: up to 36 stores per thread).
  constexpr int HALO = (PR + 1) * 4;
  for (int e = tid; e < 2 * CC * HALO; e += 256) {
    const int pl = e / HALO, h = e - pl * HALO;
    (&Ps[0][0])[pl * PLANE + (h >> 2) * RW + (h & 3)] = 0.f;
  }
  __syncthreads();

  // per-lane B base offsets (floats) for the TN column tiles
  const int dlast = NP - p0 < BN ? (int)(NP - p0) - 1 : BN - 1;  // pixels past the end of the launch read the last pixel's patch slot
  int boff[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int loc = yx0 + min(wn * WTN + j * 32 + l31, dlast);
    const int dn = loc / HW, yx = loc - dn * HW;
    const int y = yx / W, x = yx - y * W;
    boff[j] = 3 + (dn * HP + y - y0) * RW + x + half * 2 * PLANE;
  }
  // per-thread staging geometry (stage independent)
  const float* asrc[AV];
  int adst[AV];
#pragma unroll
  for (int v = 0; v < AV; ++v) {
    int u = tid + v * 256;
    if (u >= AU) u = AU - 1;                 // surplus lanes of the last pass repeat the last unit (identical stores)
    const int row = u / 9, q = u - row * 9;
    const int mr = min(m0 + row, p.Cout - 1);  // rows past Cout read row Cout-1; their outputs are never written
    asrc[v] = p.wm + (long)mr * Kp + 4 * q;
    adst[v] = 4 * q * LDA + row;
  }
  long bsrc[BV];
  int bdst[BV], bch[BV];
#pragma unroll
  for (int v = 0; v < BV; ++v) {
    int u = tid + v * 256;
    if (u >= BU) u = BU - 1;
    const int c = u / (PR * WV), rq = u - c * (PR * WV);
    const int r = rq / WV, q = rq - r * WV;
    const long rs = rowsrc[r];
    bsrc[v] = rs >= 0 ? rs + (long)c * HW + q * VEC : -1;
    bdst[v] = c * PLANE + 4 + r * RW + q * VEC;
    bch[v] = c;
  }

  f32x16 acc[TM][TN], tot[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; tot[i][j][r] = 0.f; }

  float4 ra[AV];
  float4 rb[BV];
  unsigned okb = 0;
  // staging is cut into AV+BV load pieces and AV+BV store pieces; inside the stage loop ONE piece follows each MFMA
  // group slot, so a wave's staging instructions issue while its own MFMAs execute (at 1-2 waves/SIMD the other
  // wave does not reliably cover them: ablation showed 17% of the kernel was exposed staging)
  auto load_a = [&](int v, int s) { ra[v] = *reinterpret_cast<const float4*>(asrc[v] + s * KC); };
  auto load_b = [&](int v, int s) {
    const bool ok = bsrc[v] >= 0 && s * CC + bch[v] < p.C;
    const float* src = p.x + (ok ? bsrc[v] + (long)s * CC * HW : 0);
    if (VEC == 4) {
      rb[v] = *reinterpret_cast<const float4*>(src);
    } else {
      const float2 t2 = *reinterpret_cast<const float2*>(src);
      rb[v] = make_float4(t2.x, t2.y, 0.f, 0.f);
    }
    okb = (okb & ~(1u << v)) | ((unsigned)ok << v);
  };
  auto store_a = [&](int v, int buf) {
    float* S = As[buf] + adst[v];
    S[0] = ra[v].x; S[LDA] = ra[v].y; S[2 * LDA] = ra[v].z; S[3 * LDA] = ra[v].w;
  };
  auto store_b = [&](int v, int buf) {
    const bool ok = (okb >> v) & 1;
    float* S = Ps[buf] + bdst[v];
    if (VEC == 4) *reinterpret_cast<float4*>(S) = ok ? rb[v] : make_float4(0.f, 0.f, 0.f, 0.f);
    else *reinterpret_cast<float2*>(S) = ok ? make_float2(rb[v].x, rb[v].y) : make_float2(0.f, 0.f);
  };
  constexpr int NPIECE = AV + BV;
  constexpr int KS = KC / 2;                      // MFMA k-steps per stage (18)
  constexpr int ST0 = KS - NPIECE;                // first k-step that carries a store piece
  static_assert(2 * NPIECE <= KS, "staging pieces must fit the k-steps of one stage");

#pragma unroll
  for (int v = 0; v < AV; ++v) load_a(v, 0);
#pragma unroll
  for (int v = 0; v < BV; ++v) load_b(v, 0);
#pragma unroll
  for (int v = 0; v < AV; ++v) store_a(v, 0);
#pragma unroll
  for (int v = 0; v < BV; ++v) store_b(v, 0);
  __syncthreads();
  // outer loop = one MFMA accumulation chain (SFLUSH stages): inside it the accumulators are written only by MFMAs
  // (a conditional fold inside the stage loop made hipcc move all of them between register files every stage)
  for (int s0 = 0; s0 < ns; s0 += SFLUSH) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int s1 = min(ns, s0 + SFLUSH);
    for (int s = s0; s < s1; ++s) {
      const int cur = s & 1;
      const int sn = min(s + 1, ns - 1);          // the last stage re-loads itself: keeps the body branch-free
      const float* as = As[cur] + half * LDA + wm * WTM + l31;
      const float* ps = Ps[cur];
      float a[2][TM], b[2][TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[0][i] = as[i * 32];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[0][j] = ps[boff[j]];
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        const int cb = kk & 1, nb = cb ^ 1;
        const int k1 = kk + 1, cl = k1 / 9, tap = k1 % 9;
#pragma unroll
        for (int m = 0; m < TM * TN; ++m) {
          const int i = m / TN, j = m % TN;
          acc[i][j] = mfma32(a[cb][i], b[cb][j], acc[i][j]);
          // what rides behind this MFMA
          if (m == 0 && kk + 1 < KS) {            // fragment reads of the next step: A ...
#pragma unroll
            for (int ii = 0; ii < TM; ++ii) a[nb][ii] = as[2 * k1 * LDA + ii * 32];
          }
          if (m == (TM * TN > 1 ? 1 : 0) && kk + 1 < KS) {  // ... and B
#pragma unroll
            for (int jj = 0; jj < TN; ++jj) b[nb][jj] = ps[boff[jj] + cl * PLANE + (tap / 3) * RW + (tap % 3)];
          }
          if (m == TM * TN - 1) {                 // one staging piece per k-step
            if (kk < AV) load_a(kk, sn);
            else if (kk < NPIECE) load_b(kk - AV, sn);
            else if (kk >= ST0 && kk - ST0 < AV) store_a(kk - ST0, cur ^ 1);
            else if (kk >= ST0 + AV) store_b(kk - ST0 - AV, cur ^ 1);
          }
          __builtin_amdgcn_sched_barrier(0);      // pin: hipcc would otherwise regroup loads/reads/MFMAs
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) tot[i][j] += acc[i][j];
  }

  long obase[TN];
  bool pv[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int d = wn * WTN + j * 32 + l31;
    pv[j] = d <= dlast;
    const int loc = yx0 + min(d, dlast);
    const int dn = loc / HW;
    obase[j] = (long)(n0 + dn) * p.Cout * HW + (loc - dn * HW);
  }
  igemm_epilogue<TM, TN>(tot, p, HW, m0 + __builtin_amdgcn_readfirstlane(wm) * WTM, half, obase, pv);
}

// wp[m][stage][k'] from w [Cout][Cin][3][3].  transposed = 0: m = cout, reduction channel c = cin, tap as is;
// transposed = 1 (data gradient): m = cin, c = cout, tap flipped (8 - tap).  Channels past C are zero.
__global__ void pack_weights_kernel(const float* __restrict__ w, float* __restrict__ wp, int M, int C, int CinW,
                                    int transposed) {
  const int ns = (C + V2_CC - 1) / V2_CC;
  const long total = (long)M * ns * V2_KC;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int kq = (int)(i % V2_KC);
    const long r = i / V2_KC;
    const int s = (int)(r % ns), m = (int)(r / ns);
    const int hf = kq & 1, j = kq >> 1;
    const int cl = j / 9, tap = j - cl * 9;
    const int c = s * V2_CC + cl + 2 * hf;
    float v = 0.f;
    if (c < C) v = transposed ? w[((long)c * CinW + m) * 9 + 8 - tap] : w[((long)m * CinW + c) * 9 + tap];
    wp[i] = v;
  }
}

// Grid quantisation: a layer is N*H*W/128 x Cout/128 equal workgroups on 512 resident slots (2 per CU); 1568
// workgroups are 3.06 "rounds", i.e. the last 6% of the work costs a whole round.  So the bulk (a multiple of 512
// workgroups) runs with 128x128 tiles and the remainder as 128x64 tiles (twice as many, half as long, 3 per CU).
constexpr int kSlots128 = 512;
template <int W>
void launch_v2(ConvParams p, int bn, hipStream_t s) {
  const long NP = (long)p.N * p.H * p.W;
  p.p0_base = 0; p.p_end = NP;
  if (p.Cout <= 64) {
    // 64 output channels: a 64 x 256-pixel tile gives each wave the same 72 MFMAs per stage as the 128x128 tile
    // (the 64x128 tile has half the MFMAs per staged byte and ran at ~90 instead of ~110 TFLOP/s)
    if (W >= 224 && bn != 128 && bn != 64) {
      const long ptiles = cdiv(NP, 256);
      dim3 grid((unsigned)(cdiv(ptiles, 8) * 8 * cdiv(p.Cout, 64)));
      conv3x3_igemm_v2_kernel<64, 256, W><<<grid, 256, 0, s>>>(p);
      return;
    }
    const long ptiles = cdiv(NP, 128);
    dim3 grid((unsigned)(cdiv(ptiles, 8) * 8 * cdiv(p.Cout, 64)));
    conv3x3_igemm_v2_kernel<64, 128, W><<<grid, 256, 0, s>>>(p);
    return;
  }
  const int mt = cdiv(p.Cout, 128);
  const long pt = cdiv(NP, 128);
  long pt_main = pt;
  if (bn == 64) pt_main = 0;
  else if (bn == 0 && pt * mt > kSlots128) {          // auto: peel the partial last round
    const long full = (pt * mt / kSlots128) * kSlots128;
    if (pt * mt - full > 0 && pt * mt - full <= kSlots128 * 3 / 4) pt_main = full / mt;
  }
  if (pt_main > 0) {
    ConvParams q = p;
    q.p_end = pt_main * 128 < NP ? pt_main * 128 : NP;
    dim3 grid((unsigned)(cdiv(pt_main, 8) * 8 * mt));
    conv3x3_igemm_v2_kernel<128, 128, W><<<grid, 256, 0, s>>>(q);
  }
  if (pt_main < pt) {
    ConvParams q = p;
    q.p0_base = pt_main * 128;
    dim3 grid((unsigned)(cdiv(cdiv(NP - q.p0_base, 64), 8) * 8 * mt));
    conv3x3_igemm_v2_kernel<128, 64, W><<<grid, 256, 0, s>>>(q);
  }
}

// Wt[cin][cout*9 + t] = W[cout][cin][8 - t]
__global__ void flip_transpose_kernel(const float* __restrict__ w, float* __restrict__ wt, int Cout, int Cin) {
  const long total = (long)Cout * Cin * 9;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i % 9);
    const long r = i / 9;
    const int co = (int)(r % Cout), ci = (int)(r / Cout);
    wt[i] = w[((long)co * Cin + ci) * 9 + (8 - t)];
  }
}

// ------------------------------------------------------------------------------------------------------------
// wgrad
struct WgradParams {
  const float* gz;  // [N][Cout][H][W]
  const float* x;   // [N][Cin][H][W]
  float* slab;      // [splits][9][Cout][Cin]
  float* bslab;     // [splits][Cout] or null
  int N, Cin, Cout, H, W;
  int R, CW;        // segment = R rows x CW cols (R*CW <= 32)
  int segs_y, segs_x, nsegs, segs_per_split;
};

constexpr int WG_LDG = 33;    // Gs[64][33]
constexpr int WG_PLMAX = 103;  // Xs[64][PL], PL = (R+2)*(CW+2) (+1 if even)

__global__ __launch_bounds__(256) void conv3x3_wgrad_kernel(WgradParams p) {
  __shared__ float Gs[2][64 * WG_LDG];
  __shared__ float Xs[2][64 * WG_PLMAX];
  __shared__ int pxoff[32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  const int co0 = blockIdx.y * 64, ci0 = blockIdx.x * 64;
  const int split = blockIdx.z;
  const int RW = p.CW + 2;
  const int patch = (p.R + 2) * RW;
  const int PL = patch | 1;
  const int npx = p.R * p.CW;
  const int HW = p.H * p.W;
  if (tid < 32) pxoff[tid] = tid < npx ? (tid / p.CW) * RW + (tid % p.CW) : 0;

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum[8];
#pragma unroll
  for (int v = 0; v < 8; ++v) bsum[v] = 0.f;

  const int sbeg = split * p.segs_per_split;
  const int send = min(p.nsegs, sbeg + p.segs_per_split);
  const int xs_total = 64 * patch;
  constexpr int XV = (64 * 102 + 255) / 256;  // 26 loads cover the largest patch
  float rg[8];
  float rx[XV];
  unsigned okg = 0, okx = 0;  // validity bits, applied when the registers are written to LDS

  auto load = [&](int seg) {
    okg = 0; okx = 0;
    const int sx = seg % p.segs_x;
    const int sy = (seg / p.segs_x) % p.segs_y;
    const int n = seg / (p.segs_x * p.segs_y);
    const int y0 = sy * p.R, x0 = sx * p.CW;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int e = tid + v * 256;
      const int co = e >> 5, px = e & 31;
      const int r = px / p.CW, c = px - r * p.CW;
      const bool ok = px < npx && co0 + co < p.Cout && y0 + r < p.H && x0 + c < p.W;
      rg[v] = p.gz[ok ? ((long)n * p.Cout + co0 + co) * HW + (y0 + r) * p.W + x0 + c : 0];  // branch-free
      okg |= (unsigned)ok << v;
    }
#pragma unroll
    for (int v = 0; v < XV; ++v) {
      const int e = tid + v * 256;
      const int ci = e / patch, q = e - ci * patch;
      const int rr = q / RW, cc = q - rr * RW;
      const int yy = y0 - 1 + rr, xx = x0 - 1 + cc;
      const bool ok = e < xs_total && ci0 + ci < p.Cin && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
      rx[v] = p.x[ok ? ((long)n * p.Cin + ci0 + ci) * HW + yy * p.W + xx : 0];  // branch-free
      okx |= (unsigned)ok << v;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int e = tid + v * 256;
      const float gv = ((okg >> v) & 1) ? rg[v] : 0.f;
      Gs[buf][(e >> 5) * WG_LDG + (e & 31)] = gv;
      if (p.bslab && blockIdx.x == 0) bsum[v] += gv;
    }
#pragma unroll
    for (int v = 0; v < XV; ++v) {
      const int e = tid + v * 256;
      if (e < xs_total) {
        const int ci = e / patch, q = e - ci * patch;
        Xs[buf][ci * PL + q] = ((okx >> v) & 1) ? rx[v] : 0.f;
      }
    }
  };

  if (sbeg < send) {
    load(sbeg);
    store(0);
  }
  __syncthreads();
  for (int s = sbeg; s < send; ++s) {
    const int cur = (s - sbeg) & 1;
    if (s + 1 < send) load(s + 1);
    const float* gs = Gs[cur] + (wm * 32 + l31) * WG_LDG;
    const float* xs = Xs[cur] + (wn * 32 + l31) * PL;
    // fragment reads of pixel pair kk+1 are issued before the nine MFMAs of pair kk
    float a[2], b[2][9];
    {
      a[0] = gs[kh];
      const float* xp = xs + pxoff[kh];
#pragma unroll
      for (int t = 0; t < 9; ++t) b[0][t] = xp[(t / 3) * RW + (t % 3)];
    }
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const int cb = kk & 1, nb = cb ^ 1;
      if (kk + 1 < 16) {
        const int px = 2 * (kk + 1) + kh;
        a[nb] = gs[px];
        const float* xp = xs + pxoff[px];
#pragma unroll
        for (int t = 0; t < 9; ++t) b[nb][t] = xp[(t / 3) * RW + (t % 3)];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[t] = mfma32(a[cb], b[cb][t], acc[t]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (s + 1 < send) store(cur ^ 1);
    __syncthreads();
  }

  // slab[split][t][co][ci]
#pragma unroll
  for (int t = 0; t < 9; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wm * 32 + mfma_row(r, lane);
      const int ci = ci0 + wn * 32 + l31;
      if (co < p.Cout && ci < p.Cin) p.slab[(((long)split * 9 + t) * p.Cout + co) * p.Cin + ci] = acc[t][r];
    }
  }
  if (p.bslab && blockIdx.x == 0) {
    // thread's 8 partial sums belong to couts (tid>>5)+8v; reduce over the 32 lanes sharing a cout
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      float sv = bsum[v];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) sv += __shfl_xor(sv, o, 64);
      const int co = co0 + (tid >> 5) + 8 * v;
      if ((tid & 31) == 0 && co < p.Cout) p.bslab[(long)split * p.Cout + co] = sv;
    }
  }
}

// wgrad v2: the same tiling with the segment geometry (R rows x CW columns, R*CW <= 32, CW even) as template
// parameters.  What changed against the generic kernel above, and why (rocprofv3: 7.8 VALU instructions per MFMA and
// 1 wave/SIMD left the MFMA pipe 57% idle):
//  * staging is "position owned": a thread owns one position of the (R+2)x(CW+2) halo patch (or one pixel of the gz
//    tile) and walks over channels, so an address is one add and the validity test is done once per segment;
//  * all loads are unconditional (clamped address) and the zero-select happens when the registers go to LDS;
//  * fragment addresses are per-lane base + immediate (pixel pairs never straddle a patch row because CW is even);
//  * launch bounds of 2 waves/SIMD: a second workgroup's MFMAs cover this one's staging.
template <int R, int CW>
__global__ __launch_bounds__(256, 2) void conv3x3_wgrad_v2_kernel(WgradParams p) {
  constexpr int RW = CW + 2, PP = (R + 2) * RW, PL = PP | 1, NPX = R * CW;
  constexpr int G = 256 / PP;                 // channel groups staged in parallel
  constexpr int CPG = (64 + G - 1) / G;       // channels per group = loads per thread
  static_assert((CW & 1) == 0 && NPX <= 32 && PP <= 102, "segment geometry");
  __shared__ float Gs[2][64 * WG_LDG];
  __shared__ float Xs[2][64 * PL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  const int co0 = blockIdx.y * 64, ci0 = blockIdx.x * 64;
  const int split = blockIdx.z;
  const int H = p.H, W = p.W, HW = H * W;

  // staging geometry of this thread
  const int pg = tid / PP, pos = tid - pg * PP;
  const bool pact = pg < G;
  const int prr = pos / RW, pcc = pos - prr * RW;
  const int gpx = tid & 31, gco = tid >> 5;
  const int gr = gpx / CW, gc = gpx - gr * CW;

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum[8];
#pragma unroll
  for (int v = 0; v < 8; ++v) bsum[v] = 0.f;

  const int sbeg = split * p.segs_per_split;
  const int send = min(p.nsegs, sbeg + p.segs_per_split);
  float rg[8];
  float rx[CPG];
  unsigned okg = 0, okx = 0;

  // staging in pieces (one global load or one LDS store each); inside the segment loop one piece rides behind every
  // MFMA, loads in the first slots and stores in the last, so they issue while this wave's MFMAs execute
  int cy0 = 0, cx0 = 0; long cgb = 0, cxb = 0; bool cgo = false, cxo = false;
  auto seg_setup = [&](int seg) {
    const int sx = seg % p.segs_x;
    const int sy = (seg / p.segs_x) % p.segs_y;
    const int n = seg / (p.segs_x * p.segs_y);
    cy0 = sy * R; cx0 = sx * CW;
    cgo = gpx < NPX && cy0 + gr < H && cx0 + gc < W;
    cgb = (((long)n * p.Cout + co0 + gco) * H + cy0 + gr) * W + cx0 + gc;
    const int yy = cy0 - 1 + prr, xx = cx0 - 1 + pcc;
    cxo = pact && yy >= 0 && yy < H && xx >= 0 && xx < W;
    cxb = (((long)n * p.Cin + ci0 + pg) * H + yy) * W + xx;
    okg = 0; okx = 0;
  };
  auto load_g = [&](int v) {
    const bool okv = cgo && co0 + gco + 8 * v < p.Cout;
    rg[v] = p.gz[okv ? cgb + (long)v * 8 * HW : 0];
    okg |= (unsigned)okv << v;
  };
  auto load_x = [&](int v) {
    const int ci = pg + G * v;
    const bool okv = cxo && ci < 64 && ci0 + ci < p.Cin;
    rx[v] = p.x[okv ? cxb + (long)v * G * HW : 0];
    okx |= (unsigned)okv << v;
  };
  auto store_g = [&](int v, int buf, bool fresh) {
    const float gv = ((okg >> v) & 1) ? rg[v] : 0.f;
    Gs[buf][(gco + 8 * v) * WG_LDG + gpx] = gv;
    bsum[v] += fresh ? gv : 0.f;
  };
  auto store_x = [&](int v, int buf) {
    const int ci = pg + G * v;
    if (pact && ci < 64) Xs[buf][ci * PL + pos] = ((okx >> v) & 1) ? rx[v] : 0.f;
  };
  constexpr int NP_ = 8 + CPG;                  // pieces of each kind per segment
  constexpr int NSLOT = 16 * 9;
  static_assert(2 * NP_ <= NSLOT, "pieces must fit the MFMA slots of one segment");

  if (sbeg < send) {
    seg_setup(sbeg);
#pragma unroll
    for (int v = 0; v < 8; ++v) load_g(v);
#pragma unroll
    for (int v = 0; v < CPG; ++v) load_x(v);
#pragma unroll
    for (int v = 0; v < 8; ++v) store_g(v, 0, true);
#pragma unroll
    for (int v = 0; v < CPG; ++v) store_x(v, 0);
  }
  __syncthreads();
  for (int s = sbeg; s < send; ++s) {
    const int cur = (s - sbeg) & 1;
    const bool fresh = s + 1 < send;            // the last segment re-loads itself (branch-free body), not re-counted
    seg_setup(min(s + 1, send - 1));
    const float* gs = Gs[cur] + (wm * 32 + l31) * WG_LDG + kh;
    const float* xs = Xs[cur] + (wn * 32 + l31) * PL + kh;
    float a[2], b[2][9];
    a[0] = gs[0];
#pragma unroll
    for (int t = 0; t < 9; ++t) b[0][t] = xs[(t / 3) * RW + (t % 3)];
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const int cb = kk & 1, nb = cb ^ 1;
      const int px = 2 * (kk + 1);                // even pixel of the next pair; the odd one is +1 (CW even)
      // pixels past the segment (R*CW < 32) have gz = 0; read patch offset 0 for them: anything else could touch LDS
      // that was never written and turn 0 * NaN into NaN
      const int po = px < NPX ? (px / CW) * RW + (px % CW) : 0;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        acc[t] = mfma32(a[cb], b[cb][t], acc[t]);
        if (kk + 1 < 16) {                        // next step's fragments, one read per MFMA
          if (t == 0) a[nb] = gs[px];
          b[nb][t] = xs[po + (t / 3) * RW + (t % 3)];
        }
        const int q = kk * 9 + t;                 // staging piece of this slot
        if (q < 8) load_g(q);
        else if (q < NP_) load_x(q - 8);
        else if (q >= NSLOT - NP_ && q < NSLOT - CPG) store_g(q - (NSLOT - NP_), cur ^ 1, fresh);
        else if (q >= NSLOT - CPG) store_x(q - (NSLOT - CPG), cur ^ 1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int t = 0; t < 9; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wm * 32 + mfma_row(r, lane);
      const int ci = ci0 + wn * 32 + l31;
      if (co < p.Cout && ci < p.Cin) p.slab[(((long)split * 9 + t) * p.Cout + co) * p.Cin + ci] = acc[t][r];
    }
  }
  if (p.bslab && blockIdx.x == 0) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      float sv = bsum[v];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) sv += __shfl_xor(sv, o, 64);
      const int co = co0 + gco + 8 * v;
      if (gpx == 0 && co < p.Cout) p.bslab[(long)split * p.Cout + co] = sv;
    }
  }
}

// wgrad for Cin <= 3 (the first VGG layer, RGB input): the 9*Cin <= 27 (channel, tap) pairs become the 32 columns
// of ONE accumulator tile instead of nine tiles with 3 of 32 columns in use.  Lane j = ci*9 + tap reads the patch at
// ci*PL + (tap/3)*RW + tap%3 (+ pixel offset as an immediate); lanes >= 9*Cin compute garbage that is never stored.
// Segment geometry R x CW as in the general kernel.  64 cout per workgroup: wave w owns couts 32*(w&1).. and pixel
// pairs of parity (w>>1) (two half-K chains, summed through LDS at the end).
template <int R, int CW>
__global__ __launch_bounds__(256) void conv3x3_wgrad_c3_kernel(WgradParams p) {
  constexpr int RW = CW + 2, PP = (R + 2) * RW, PL = PP | 1, NPX = R * CW;
  static_assert((CW & 1) == 0 && NPX <= 32 && PP <= 102, "segment geometry");
  __shared__ float Gs[2][64 * WG_LDG];
  __shared__ float Xs[2][4 * PL];
  __shared__ float Red[2][32 * 33];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wk = wave >> 1;
  const int l31 = lane & 31, kh = lane >> 5;
  const int co0 = blockIdx.y * 64;
  const int split = blockIdx.z;
  const int H = p.H, W = p.W, HW = H * W;
  const int gpx = tid & 31, gco = tid >> 5;
  const int gr = gpx / CW, gc = gpx - gr * CW;
  // patch staging: thread -> (channel, position), 3*PP <= 306 elements: two passes
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float bsum[8];
#pragma unroll
  for (int v = 0; v < 8; ++v) bsum[v] = 0.f;
  const int sbeg = split * p.segs_per_split;
  const int send = min(p.nsegs, sbeg + p.segs_per_split);
  float rg[8], rx[2];
  unsigned okg = 0, okx = 0;
  auto load = [&](int seg) {
    const int sx = seg % p.segs_x;
    const int sy = (seg / p.segs_x) % p.segs_y;
    const int n = seg / (p.segs_x * p.segs_y);
    const int y0 = sy * R, x0 = sx * CW;
    okg = 0; okx = 0;
    const bool ok = gpx < NPX && y0 + gr < H && x0 + gc < W;
    const long base = (((long)n * p.Cout + co0 + gco) * H + y0 + gr) * W + x0 + gc;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const bool okv = ok && co0 + gco + 8 * v < p.Cout;
      rg[v] = p.gz[okv ? base + (long)v * 8 * HW : 0];
      okg |= (unsigned)okv << v;
    }
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int e = tid + 256 * v;
      const int ci = e / PP, pos = e - ci * PP;
      const int prr = pos / RW, pcc = pos - prr * RW;
      const int yy = y0 - 1 + prr, xx = x0 - 1 + pcc;
      const bool okv = ci < p.Cin && yy >= 0 && yy < H && xx >= 0 && xx < W;
      rx[v] = p.x[okv ? (((long)n * p.Cin + ci) * H + yy) * W + xx : 0];
      okx |= (unsigned)okv << v;
    }
  };
  auto store = [&](int buf, bool fresh) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const float gv = ((okg >> v) & 1) ? rg[v] : 0.f;
      Gs[buf][(gco + 8 * v) * WG_LDG + gpx] = gv;
      bsum[v] += fresh ? gv : 0.f;
    }
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int e = tid + 256 * v;
      const int ci = e / PP, pos = e - ci * PP;
      if (ci < 4) Xs[buf][ci * PL + pos] = ((okx >> v) & 1) ? rx[v] : 0.f;
    }
  };
  // lane's (channel, tap) column
  const int jc = l31 / 9, jt = l31 - jc * 9;
  const int xcol = (jc < 3 ? jc : 3) * PL + (jt / 3) * RW + (jt % 3) + kh;
  if (sbeg < send) { load(sbeg); store(0, true); }
  __syncthreads();
  for (int s = sbeg; s < send; ++s) {
    const int cur = (s - sbeg) & 1;
    load(min(s + 1, send - 1));
    const float* gs = Gs[cur] + (wm * 32 + l31) * WG_LDG + kh;
    const float* xs = Xs[cur] + xcol;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int kk = 2 * q + wk;                   // this wave's half of the 16 pixel pairs
      const int px = 2 * kk;
      const int po = (px / CW) * RW + (px % CW);
      // wk is wave-uniform but not a compile-time constant: both candidates are immediates, select by wk
      const int px0 = 2 * (2 * q), px1 = 2 * (2 * q + 1);
      const int po0 = (px0 / CW) * RW + (px0 % CW), po1 = (px1 / CW) * RW + (px1 % CW);
      const float a = wk ? gs[px1] : gs[px0];
      const float b = wk ? xs[po1] : xs[po0];
      (void)px; (void)po;
      acc = mfma32(a, b, acc);
    }
    store(cur ^ 1, s + 1 < send);
    __syncthreads();
  }
  // combine the two pixel-parity chains: waves 2,3 -> LDS -> waves 0,1
  if (wk == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) Red[wm][mfma_row(r, lane) * 33 + l31] = acc[r];
  }
  __syncthreads();
  if (wk == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mfma_row(r, lane);
      const float v = acc[r] + Red[wm][row * 33 + l31];
      const int co = co0 + wm * 32 + row;
      if (co < p.Cout && jc < p.Cin && l31 < 9 * p.Cin)
        p.slab[(((long)split * 9 + jt) * p.Cout + co) * p.Cin + jc] = v;
    }
  }
  if (p.bslab) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      float sv = bsum[v];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) sv += __shfl_xor(sv, o, 64);
      const int co = co0 + gco + 8 * v;
      if (gpx == 0 && co < p.Cout) p.bslab[(long)split * p.Cout + co] = sv;
    }
  }
}

// dW[co][ci][t] (+)= sum_split slab[split][t][co][ci];  db[co] (+)= sum_split bslab[split][co]
__global__ void wgrad_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bslab, int splits,
                                    int Cout, int Cin, float* __restrict__ dw, float* __restrict__ db, int accumulate) {
  const long per = (long)9 * Cout * Cin;
  const long total = per + (bslab ? Cout : 0);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    if (i < per) {
      float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
      int s = 0;
      for (; s + 3 < splits; s += 4) {
        v0 += slab[(long)s * per + i]; v1 += slab[(long)(s + 1) * per + i];
        v2 += slab[(long)(s + 2) * per + i]; v3 += slab[(long)(s + 3) * per + i];
      }
      for (; s < splits; ++s) v0 += slab[(long)s * per + i];
      const float v = (v0 + v1) + (v2 + v3);
      const int ci = (int)(i % Cin);
      const long r = i / Cin;
      const int co = (int)(r % Cout), t = (int)(r / Cout);
      float* d = dw + ((long)co * Cin + ci) * 9 + t;
      *d = accumulate ? *d + v : v;
    } else {
      const int co = (int)(i - per);
      float v = 0.f;
      for (int s = 0; s < splits; ++s) v += bslab[(long)s * Cout + co];
      db[co] = accumulate ? db[co] + v : v;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// 2x2/2 max pooling, and its backward fused with the ReLU mask of the (post-ReLU) pooled input
__global__ void maxpool2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long planes, int H, int W) {
  const int Ho = H / 2, Wo = W / 2;
  const long total = planes * Ho * Wo;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wo);
    const long r = i / Wo;
    const int yo = (int)(r % Ho);
    const long pl = r / Ho;
    const float* s = x + (pl * H + 2 * yo) * W + 2 * xo;
    const float2 a = *reinterpret_cast<const float2*>(s);
    const float2 b = *reinterpret_cast<const float2*>(s + W);
    y[i] = fmaxf(fmaxf(a.x, a.y), fmaxf(b.x, b.y));
  }
}

// gx = route(gy) to the first maximum of each window, zeroed where the maximum is not > 0 (ReLU backward of
// the activation that fed the pool)
__global__ void maxpool2_bwd_relu_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                         float* __restrict__ gx, long planes, int H, int W) {
  const int Ho = H / 2, Wo = W / 2;
  const long total = planes * Ho * Wo;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wo);
    const long r = i / Wo;
    const int yo = (int)(r % Ho);
    const long pl = r / Ho;
    const long o = (pl * H + 2 * yo) * W + 2 * xo;
    const float2 a = *reinterpret_cast<const float2*>(x + o);
    const float2 b = *reinterpret_cast<const float2*>(x + o + W);
    int arg = 0;
    float m = a.x;
    if (a.y > m) { m = a.y; arg = 1; }
    if (b.x > m) { m = b.x; arg = 2; }
    if (b.y > m) { m = b.y; arg = 3; }
    const float g = m > 0.f ? gy[i] : 0.f;
    float2 ga = make_float2(arg == 0 ? g : 0.f, arg == 1 ? g : 0.f);
    float2 gb = make_float2(arg == 2 ? g : 0.f, arg == 3 ? g : 0.f);
    *reinterpret_cast<float2*>(gx + o) = ga;
    *reinterpret_cast<float2*>(gx + o + W) = gb;
  }
}

}  // namespace

// ---- internal host entry points ------------------------------------------------------------------------------
// UMPR_CONV_BN: 0 auto (128x128 bulk + 128x64 tail), 128 or 64 force one tile shape (A/B runs)
static int conv_bn() { static const int v = umpr_env_int("UMPR_CONV_BN", 0); return v; }
// ---- first layer (Cin <= 3): no LDS, no barriers.  K = 27 is too short for the staged kernels (they pad it to a
// 144-deep stage and become MFMA-bound on zeros); here every wave keeps its weight fragments in registers for the
// whole launch and walks over 32-pixel tiles: 14 gathered loads per lane (image planes stay in L2), 14 MFMA k-steps
// for each 32-channel block, +bias, ReLU, 128-B row-segment stores.  The launch is bound by the output write.
template <int TM>   // TM = Cout / 32
__global__ __launch_bounds__(256) void conv3x3_fwd_c3_kernel(ConvParams p) {
  constexpr int KS = 14;   // k = 2 * kk + half < 28; k = c * 9 + tap, k >= C * 9 contributes zero
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * 4;
  const int KR = p.C * 9;
  float wa[TM][KS];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int k = 2 * kk + half;
      wa[i][kk] = k < KR ? p.wm[(long)(i * 32 + l31) * KR + k] : 0.f;
    }
  float bv[TM][16];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) bv[i][r] = p.bias ? p.bias[i * 32 + mfma_row(r, lane)] : 0.f;
  const long HW = (long)p.H * p.W;
  const long ntiles = (p.p_end + 31) / 32;
  for (long t = wave; t < ntiles; t += nwaves) {
    const long px = t * 32 + l31;
    const bool okp = px < p.p_end;
    const long pc = okp ? px : 0;
    const int n = (int)(pc / HW);
    const int rem = (int)(pc - (long)n * HW);
    const int y = rem / p.W, x = rem - y * p.W;
    const float* img = p.x + (long)n * p.C * HW;
    float b[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int k = 2 * kk + half;
      const int c = k / 9, tap = k - c * 9;
      const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
      const bool ok = okp && k < KR && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
      const float v = img[ok ? (long)c * HW + (long)yy * p.W + xx : 0];
      b[kk] = ok ? v : 0.f;
    }
    f32x16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = bv[i][r];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
      for (int i = 0; i < TM; ++i) acc[i] = mfma32(wa[i][kk], b[kk], acc[i]);
    if (okp) {
      float* out = p.y + (long)n * p.Cout * HW + rem;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[i][r];
          if (p.relu) v = fmaxf(v, 0.f);
          out[(long)(i * 32 + mfma_row(r, lane)) * HW] = v;
        }
    }
  }
}

// ---- the plan --------------------------------------------------------------------------------------------------
// Which kernels a pass of a layer runs (D = LDS-patch direct kernels, C = first-layer kernels, G = generic gather kernels,
// W2 / W4 = Winograd on the F(2x2,3x3) / F(4x4,3x3) tile), by UMPR_WINO_F4 = 2 (default) | 1 | 0.  "Reduction channels" are
// Cin in forward, Cout in the data gradient; the weight gradient wants 32 channels on both sides.
//
//   layer class                                   forward (training)  forward (inference)  data gradient   weight gradient
//   Cin <= 3, Cout = 64 (conv1_1)                 C                   C                    D, else G       C (W % 16 == 0)
//   56 / 28 / 14 maps, >= 32 reduction channels   W4 | W2 | W2        W4 | W4 | W2         W4 | W4 | W2    W4 | W4 | W2 (14: W2)
//   112 map, >= 128 channels both sides (conv2_2) W4 | D  | D         W4 | W4 | D          W4 | W4 | D     W4 | W4 | D
//   112 map, Cin >= 64, Cout >= 128 (conv2_1)     D                   W4 | W4 | D          D               W4 | W4 | D
//   other 224 / 112 / 56 / 28 / 14 maps           D                   D                    D               D
//   any other shape                               G                   G                    G               G (D: W % 8 or % 14 == 0)
//
// Why, row by row.  The 4x4 tile does 4x fewer MFMA FLOPs than the direct kernel (the 2x2 tile 2.25x) and pays where 36 planes
// over ceil(H/4) x ceil(W/4) tiles are less GEMM work than 16 planes over (H/2) x (W/2) - on 14x14 too, where 3.75 of 16 tiles hang
// over the border (`edge`).  Its rounding (1-2e-6 of max|y|) is a smooth perturbation in backward, which is linear in its inputs
// (mode 1); a training forward takes it since the decision fix-up retakes every ReLU / pool decision it could change (mode 2),
// and an inference forward (ConvHints::inference) has no backward pass reading its decisions.  The weight gradient of the
// padded 14x14 maps stays on the 2x2 tile: a quarter of the tiles is too short a reduction for the split-K GEMM and the 36-plane
// finish (0.367 vs 0.353 ms per layer).  At 112x112 only the 4x4 tile pays (with the 2x2 one the 4x activation-sized transform
// traffic ate the gain), so those rows follow UMPR_WINO_112 (default: on in modes >= 1) and the training forward of conv2_2
// UMPR_WINO_112_FWD.  conv2_1 has 64 reduction channels in forward: two K stages, bound by V / M traffic, still ahead of the
// direct kernel (30.9 vs 31.36 ms per step) - but in training its rounding enters the chain one layer earlier and two more ReLU
// decisions of the golden fixture umpr_full_V1_B2 fall on the other side of float64 (conv1_1 weight gradient 1.5e-2 from the
// reference, bound 6e-3; tools/count_flips.py --fixture 51,52,2 --chained), so only inference takes it unless
// UMPR_WINO_C21_FWD = 1 (0: never); its data gradient would write half a GEMM row tile of padding and stays direct.
// UMPR_CONV_WINO = 0 keeps forward and data gradient off Winograd, UMPR_WGRAD_WINO = 0 the weight gradient, UMPR_CONV_V1 = 1
// puts every pass on the generic kernels (A/B runs).
//
// ws_floats is what a caller reserves for the pass, and what the public size entry points add up.  For a planned Winograd
// pass it is the Winograd workspace (never smaller than the packed weights); the launcher falls back to plan.direct when the
// caller brings less and names no V slot.  Two of its terms are only sized for, never reached, and kept because sizes must
// not move: (1) a forward sizes for the larger of the 2x2 and the 4x4 geometry in modes >= 1; mode 1 reaches both (training,
// inference), mode 2 only the 4x4 one, so the 2x2 term - the larger, which governs umpr_conv3x3_pack_bytes - is never reached
// by default; (2) it is taken by map size alone, so a layer with fewer than 32 reduction channels, or any layer under
// UMPR_CONV_V1 = 1, reserves a Winograd workspace it cannot use.
//
// v_floats: the training forward (W4, no edge tiles) computes exactly the transformed input V that the weight gradient of the
// same layer (W4, same padded channel count) would compute again; both plans then name the size of the slot they share
// (UMPR_WINO_V_REUSE = 0: never).  Seven of the thirteen VGG16 layers qualify.
namespace {
struct ConvSwitches { bool wino, v1, wgrad_wino, w112, w112_fwd, v_reuse; int f4, c21_fwd; };
ConvSwitches read_conv_switches() {
  ConvSwitches v;
  v.wino = umpr_env_on("UMPR_CONV_WINO");
  v.v1 = umpr_env_int("UMPR_CONV_V1", 0) == 1;
  v.wgrad_wino = umpr_env_on("UMPR_WGRAD_WINO");
  v.f4 = umpr_env_int("UMPR_WINO_F4", 2);
  const int w112 = umpr_env_int("UMPR_WINO_112", -1);
  v.w112 = w112 == 1 || (w112 < 0 && v.f4 >= 1);
  v.w112_fwd = umpr_env_int("UMPR_WINO_112_FWD", 1) != 0;
  v.c21_fwd = umpr_env_int("UMPR_WINO_C21_FWD", -1);
  v.v_reuse = umpr_env_int("UMPR_WINO_V_REUSE", 1) != 0;
  return v;
}
const ConvSwitches& conv_switches() { static const ConvSwitches v = read_conv_switches(); return v; }

// pixel segment of the direct weight gradient = R rows x CW columns with R*CW <= 32: full MFMA k-utilisation when W is a
// multiple of 32/16/8
void wgrad_segment(int W, int* R, int* CW) {
  // two-row segments keep the halo patch small (72 / 64 positions -> 22 / 16 loads per thread and no register spills;
  // the one-row 32- and 28-wide variants needed 32 loads and spilled)
  if (W % 16 == 0) { *R = 2; *CW = 16; }
  else if (W % 8 == 0) { *R = 4; *CW = 8; }
  else if (W % 14 == 0) { *R = 2; *CW = 14; }
  else if (W < 32) { *R = 32 / W; *CW = W; }
  else { *R = 1; *CW = 32; }
}

struct LayerClass { bool deep, c22, c21, f4_shape; };
LayerClass layer_class(int Cin, int Cout, int H, int W) {
  const bool at112 = conv_switches().w112 && H == 112 && W == 112;
  return {H == W && (W == 56 || W == 28 || W == 14), at112 && Cin >= 128 && Cout >= 128, at112 && Cin >= 64 && Cout >= 128,
          36L * ((H + 3) / 4) * ((W + 3) / 4) < 16L * (H / 2) * (W / 2)};
}

// the kernels of a pass that is not on Winograd
ConvAlgo direct_algo(ConvPass pass, int Cin, int Cout, int H, int W) {
  if (conv_switches().v1) return CONV_GENERIC;
  if (pass == CONV_WGRAD) {
    int R, CW;
    wgrad_segment(W, &R, &CW);
    if (R == 2 && CW == 16) return Cin <= 3 ? CONV_C3 : CONV_DIRECT;
    return (R == 4 && CW == 8) || (R == 2 && CW == 14) ? CONV_DIRECT : CONV_GENERIC;
  }
  if (pass == CONV_FWD && Cin <= 3 && Cout == 64) return CONV_C3;
  return H == W && (W == 224 || W == 112 || W == 56 || W == 28 || W == 14) ? CONV_DIRECT : CONV_GENERIC;
}

ConvAlgo conv_algo(ConvPass pass, int Cin, int Cout, int H, int W, bool inference) {
  const ConvSwitches& sw = conv_switches();
  const LayerClass lc = layer_class(Cin, Cout, H, W);
  bool wino, f4 = sw.f4 >= 1 && lc.f4_shape;
  if (pass == CONV_FWD) {
    const bool inf = inference && sw.f4 >= 1;
    const bool wide = inf || (sw.w112_fwd && sw.f4 >= 2);   // the 112 rows are open to this forward
    const bool c21 = lc.c21 && (sw.c21_fwd == 1 || (sw.c21_fwd < 0 && inf));
    wino = sw.wino && Cin >= 32 && (lc.deep || (wide && (lc.c22 || c21)));
    f4 = f4 && (inf || sw.f4 >= 2);
  } else if (pass == CONV_DGRAD) {
    wino = sw.wino && Cout >= 32 && (lc.deep || lc.c22);
  } else {
    wino = sw.wgrad_wino && Cin >= 32 && Cout >= 32 && (lc.deep || lc.c22 || lc.c21);
    f4 = f4 && (H % 4) == 0 && (W % 4) == 0;
  }
  if (!wino || sw.v1) return direct_algo(pass, Cin, Cout, H, W);
  return f4 ? CONV_WINO4 : CONV_WINO2;
}

constexpr int kWgradTargetWgs = 512;  // workgroups per wgrad launch (2 resident per CU): split-K factor = this / tiles
// Segments and split-K plan of the direct weight gradient; the slabs are [splits][9][Cout][Cin] + [splits][Cout]
struct WgradGeom { int R, CW, segs_y, segs_x, nsegs, splits, segs_per_split; size_t per_split, bytes; };
WgradGeom wgrad_geom(int N, int Cin, int Cout, int H, int W) {
  WgradGeom g;
  wgrad_segment(W, &g.R, &g.CW);
  g.segs_y = cdiv(H, g.R); g.segs_x = cdiv(W, g.CW); g.nsegs = N * g.segs_y * g.segs_x;
  g.splits = cdiv(kWgradTargetWgs, cdiv(Cout, 64) * cdiv(Cin, 64));
  if (g.splits > g.nsegs) g.splits = g.nsegs;
  g.segs_per_split = cdiv(g.nsegs, g.splits);
  g.per_split = ((size_t)9 * Cout * Cin + Cout) * sizeof(float);
  g.bytes = (size_t)g.splits * g.per_split;
  return g;
}
}  // namespace

ConvPlan umpr_conv3x3_plan(ConvPass pass, int N, int Cin, int Cout, int H, int W, bool inference) {
  const ConvSwitches& sw = conv_switches();
  const LayerClass lc = layer_class(Cin, Cout, H, W);
  ConvPlan p;
  p.algo = conv_algo(pass, Cin, Cout, H, W, inference);
  p.direct = direct_algo(pass, Cin, Cout, H, W);
  p.edge = p.algo == CONV_WINO4 && ((H % 4) != 0 || (W % 4) != 0);
  p.v_floats = 0;
  const bool wino = p.algo == CONV_WINO2 || p.algo == CONV_WINO4;
  if (pass == CONV_WGRAD) {
    p.ws_floats = wino ? umpr_wino_wgrad_geom(N, Cin, Cout, H, W, p.algo == CONV_WINO4).floats
                       : wgrad_geom(N, Cin, Cout, H, W).bytes / sizeof(float);
  } else {
    const int M = pass == CONV_DGRAD ? Cin : Cout, C = pass == CONV_DGRAD ? Cout : Cin;
    p.ws_floats = (size_t)M * ((C + V2_CC - 1) / V2_CC) * V2_KC;   // packed weights (>= the generic kernel's flip-transpose)
    const bool c21_possible = pass == CONV_FWD && lc.c21 && sw.c21_fwd != 0;
    if (sw.wino && (lc.deep || lc.c22 || c21_possible)) {   // sized by map alone, see (2) above
      const bool f4 = sw.f4 >= 1 && lc.f4_shape;
      size_t f = umpr_wino_conv_geom(N, C, M, H, W, f4).floats;
      if (f4 && pass == CONV_FWD) {                          // both tiles, see (1) above
        const size_t f2 = umpr_wino_conv_geom(N, C, M, H, W, false).floats;
        if (f2 > f) f = f2;
      }
      if (f > p.ws_floats) p.ws_floats = f;
    }
  }
  // (a weight gradient on the 4x4 tile has no edge tiles, so neither has the forward that shares its V)
  if (pass != CONV_DGRAD && !(pass == CONV_FWD && inference) && sw.v_reuse &&
      conv_algo(CONV_FWD, Cin, Cout, H, W, false) == CONV_WINO4 && conv_algo(CONV_WGRAD, Cin, Cout, H, W, false) == CONV_WINO4) {
    const WinoConvGeom fg = umpr_wino_conv_geom(N, Cin, Cout, H, W, true);
    const WinoWgradGeom wg = umpr_wino_wgrad_geom(N, Cin, Cout, H, W, true);
    if (fg.v_floats == (size_t)wg.planes * wg.Cpad * wg.Tpad) p.v_floats = fg.v_floats;   // the two GEMMs pad the channels alike
  }
  return p;
}

// scratch floats the forward and the data gradient of a layer need: the packed weights, or the Winograd U / V / M buffers
size_t umpr_conv3x3_pack_floats(int N, int Cin, int Cout, int H, int W) {
  const size_t f = umpr_conv3x3_plan(CONV_FWD, N, Cin, Cout, H, W, false).ws_floats;
  const size_t t = umpr_conv3x3_plan(CONV_DGRAD, N, Cin, Cout, H, W, false).ws_floats;
  return f > t ? f : t;
}

// Whether the two gradients of a layer that a 2x2 max-pool follows can read the POOLED gradient (ConvHints::pooled_dy): the data
// gradient's reader is wino4_input_kernel, the weight gradient's wino4_dy_kernel (no edge tiles by its plan) or wino_dy[_pair]_kernel.
// Any other plan (the direct kernels of conv1_2, the 2x2 tile's data gradient under UMPR_WINO_F4 = 0) has no such reader and its
// caller runs umpr_maxpool2_bwd_relu_impl first.  UMPR_POOL_FOLD = 0: never (the sequence of kernels before the fold existed).
bool umpr_conv3x3_pool_fold_ok(int N, int Cin, int Cout, int H, int W) {
  static const bool on = umpr_env_on("UMPR_POOL_FOLD");
  if (!on || (H % 2) != 0 || (W % 2) != 0) return false;
  const ConvAlgo wg = umpr_conv3x3_plan(CONV_WGRAD, N, Cin, Cout, H, W, false).algo;
  return umpr_conv3x3_plan(CONV_DGRAD, N, Cin, Cout, H, W, false).algo == CONV_WINO4 && (wg == CONV_WINO4 || wg == CONV_WINO2);
}

// Forward (transposed = 0):  y[N][Cout] = relu?(conv(x[N][Cin], w) + bias)
// Data gradient (transposed = 1):  y[N][Cin] = conv^T(x[N][Cout], w) * [mask > 0]
// w is always the parameter [Cout][Cin][3][3]; wpack: scratch of umpr_conv3x3_pack_floats(...) floats.
int umpr_conv3x3_run(const float* x, const float* w, int transposed, const float* bias, const float* mask, float* y,
                     int N, int Cin, int Cout, int H, int W, int relu, float* wpack, size_t wpack_floats,
                     const ConvHints& hints, hipStream_t s) {
  UMPR_REQUIRE(N > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0, "conv3x3: bad shape");
  UMPR_REQUIRE(transposed || !mask, "conv3x3: the forward pass takes no mask");
  const int M = transposed ? Cin : Cout;   // output channels of this launch
  const int C = transposed ? Cout : Cin;   // reduction channels
  const long NP = (long)N * H * W;
  const ConvPlan plan = umpr_conv3x3_plan(transposed ? CONV_DGRAD : CONV_FWD, N, Cin, Cout, H, W, hints.inference);
  ConvAlgo algo = plan.algo;
  const bool fits = wpack && wpack_floats >= plan.ws_floats;
  if (hints.v_slot)   // the weight gradient will read the slot: this call must be the one that writes it
    UMPR_REQUIRE(algo == CONV_WINO4 && fits && plan.v_floats > 0 && plan.v_floats == hints.v_slot_floats,
                 "conv3x3: the V slot does not fit this call (%d -> %d at %dx%d, slot %zu floats, plan %zu)", Cin, Cout, H, W,
                 hints.v_slot_floats, plan.v_floats);
  else if ((algo == CONV_WINO2 || algo == CONV_WINO4) && !fits) algo = plan.direct;   // scratch of a direct call only
  if (hints.pooled_dy)   // only wino4_input_kernel can read a pooled gradient: the caller asked umpr_conv3x3_pool_fold_ok first
    UMPR_REQUIRE(transposed && algo == CONV_WINO4 && hints.pool_y, "conv3x3: no reader with a pooled source for this call (%d -> %d at %dx%d)",
                 Cin, Cout, H, W);
  if (algo == CONV_DIRECT && !wpack) algo = CONV_GENERIC;                             // a forward without scratch
  const int family = transposed ? UMPR_K_CONV_DGRAD : UMPR_K_CONV_IGEMM;   // one family for every algorithm, with the direct
  const double work = 2.0 * NP * M * C * 9;                                // conv's FLOP count
  switch (algo) {
    case CONV_WINO2:
    case CONV_WINO4: {
      UmprProfScope prof(family, work, s);
      return umpr_wino_conv3x3(x, w, transposed, bias, mask, y, N, Cin, Cout, H, W, relu, wpack, wpack_floats,
                               algo == CONV_WINO4, hints, s);
    }
    case CONV_C3: {
      ConvParams p{x, w, bias, nullptr, y, N, Cin, H, W, Cout, relu, 0, NP};
      UmprProfScope prof(family, work, s);
      conv3x3_fwd_c3_kernel<2><<<2048, 256, 0, s>>>(p);
      UMPR_LAUNCH_CHECK("conv3x3_fwd_c3");
      return 0;
    }
    case CONV_DIRECT: {
      const long total = (long)M * ((C + V2_CC - 1) / V2_CC) * V2_KC;
      UMPR_REQUIRE(wpack_floats >= (size_t)total, "conv3x3: weight scratch too small");
      // the kernels take their whole geometry from the template width
      UMPR_REQUIRE(H == W && (W == 224 || W == 112 || W == 56 || W == 28 || W == 14), "conv3x3: the direct kernels need a square VGG map, not %dx%d", H, W);
      int blocks = (int)((total + 255) / 256);
      if (blocks > 4096) blocks = 4096;
      pack_weights_kernel<<<blocks, 256, 0, s>>>(w, wpack, M, C, Cin, transposed);
      UMPR_LAUNCH_CHECK("pack_weights");
      ConvParams p{x, wpack, bias, mask, y, N, C, H, W, M, relu, 0, NP};
      UmprProfScope prof(family, work, s);
      if (W == 224) launch_v2<224>(p, conv_bn(), s);
      else if (W == 112) launch_v2<112>(p, conv_bn(), s);
      else if (W == 56) launch_v2<56>(p, conv_bn(), s);
      else if (W == 28) launch_v2<28>(p, conv_bn(), s);
      else launch_v2<14>(p, conv_bn(), s);
      UMPR_LAUNCH_CHECK("conv3x3_igemm_v2");
      return 0;
    }
    case CONV_GENERIC: break;
  }
  const float* wm = w;
  if (transposed) {
    UMPR_REQUIRE(wpack != nullptr && wpack_floats >= (size_t)Cin * Cout * 9, "conv3x3: data gradient needs the weight scratch");
    if (int rc = umpr_conv3x3_flip_transpose(w, wpack, Cout, Cin, s)) return rc;
    wm = wpack;
  }
  ConvParams p{x, wm, bias, mask, y, N, C, H, W, M, relu, 0, NP};
  UmprProfScope prof(family, work, s);
  if (M <= 64) {
    dim3 grid(cdiv(NP, 128), cdiv(M, 64));
    conv3x3_igemm_kernel<64, 128><<<grid, 256, 0, s>>>(p);
  } else {
    dim3 grid(cdiv(NP, 128), cdiv(M, 128));
    conv3x3_igemm_kernel<128, 128><<<grid, 256, 0, s>>>(p);
  }
  UMPR_LAUNCH_CHECK("conv3x3_igemm");
  return 0;
}

int umpr_conv3x3_flip_transpose(const float* w, float* wt, int Cout, int Cin, hipStream_t s) {
  const long total = (long)Cout * Cin * 9;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  flip_transpose_kernel<<<blocks, 256, 0, s>>>(w, wt, Cout, Cin);
  UMPR_LAUNCH_CHECK("flip_transpose");
  return 0;
}

size_t umpr_conv3x3_wgrad_ws_bytes(int N, int Cin, int Cout, int H, int W) {
  return umpr_conv3x3_plan(CONV_WGRAD, N, Cin, Cout, H, W, false).ws_floats * sizeof(float);
}

int umpr_conv3x3_wgrad(const float* gz, const float* x, float* dw, float* db, int N, int Cin, int Cout, int H, int W,
                       int accumulate, float* ws, size_t ws_bytes, const ConvHints& hints, hipStream_t s) {
  const ConvPlan plan = umpr_conv3x3_plan(CONV_WGRAD, N, Cin, Cout, H, W, false);
  ConvAlgo algo = plan.algo;
  const bool fits = ws_bytes >= plan.ws_floats * sizeof(float);
  if (hints.v_slot)   // "written by the forward" holds only if that forward ran the plan this call runs
    UMPR_REQUIRE(algo == CONV_WINO4 && fits && plan.v_floats > 0 && plan.v_floats == hints.v_slot_floats,
                 "conv3x3 wgrad: the V slot does not match this layer (%d -> %d at %dx%d, slot %zu floats, plan %zu)", Cin, Cout,
                 H, W, hints.v_slot_floats, plan.v_floats);
  else if ((algo == CONV_WINO2 || algo == CONV_WINO4) && !fits) algo = plan.direct;   // workspace of a direct call only
  if (hints.pooled_dy)   // only the Winograd dy transforms can read a pooled gradient
    UMPR_REQUIRE((algo == CONV_WINO2 || algo == CONV_WINO4) && hints.pool_y,
                 "conv3x3 wgrad: no reader with a pooled source for this call (%d -> %d at %dx%d)", Cin, Cout, H, W);
  const double work = 2.0 * N * H * W * Cout * Cin * 9;   // one family for every algorithm, with the direct algorithm's FLOP count
  if (algo == CONV_WINO2 || algo == CONV_WINO4) {
    UmprProfScope prof(UMPR_K_CONV_WGRAD, work, s);
    return umpr_wino_wgrad(gz, x, dw, db, N, Cin, Cout, H, W, accumulate, ws, ws_bytes / sizeof(float), algo == CONV_WINO4, hints, s);
  }
  const WgradGeom g = wgrad_geom(N, Cin, Cout, H, W);
  UMPR_REQUIRE(g.R * g.CW <= 32 && (g.R + 2) * (g.CW + 2) <= 102, "wgrad: unsupported width %d", W);
  WgradParams p;
  p.gz = gz; p.x = x; p.N = N; p.Cin = Cin; p.Cout = Cout; p.H = H; p.W = W;
  p.R = g.R; p.CW = g.CW; p.segs_y = g.segs_y; p.segs_x = g.segs_x; p.nsegs = g.nsegs; p.segs_per_split = g.segs_per_split;
  if (g.bytes > ws_bytes) {   // a smaller workspace: fewer, longer splits
    const int fit = (int)(ws_bytes / g.per_split);
    UMPR_REQUIRE(fit >= 1, "wgrad: workspace too small (%zu bytes)", ws_bytes);
    p.segs_per_split = cdiv(g.nsegs, fit);
  }
  const int splits = cdiv(p.nsegs, p.segs_per_split);
  p.slab = ws;
  p.bslab = db ? ws + (size_t)splits * 9 * Cout * Cin : nullptr;
  dim3 grid(cdiv(Cin, 64), cdiv(Cout, 64), splits);
  {
    UmprProfScope prof(UMPR_K_CONV_WGRAD, work, s);
    switch (algo) {
      case CONV_C3: conv3x3_wgrad_c3_kernel<2, 16><<<grid, 256, 0, s>>>(p); break;
      case CONV_DIRECT:
        if (g.R == 2 && g.CW == 16) conv3x3_wgrad_v2_kernel<2, 16><<<grid, 256, 0, s>>>(p);
        else if (g.R == 4) conv3x3_wgrad_v2_kernel<4, 8><<<grid, 256, 0, s>>>(p);
        else conv3x3_wgrad_v2_kernel<2, 14><<<grid, 256, 0, s>>>(p);
        break;
      default: conv3x3_wgrad_kernel<<<grid, 256, 0, s>>>(p);
    }
  }
  UMPR_LAUNCH_CHECK("conv3x3_wgrad");
  return umpr_wgrad_reduce(p.slab, p.bslab, splits, Cout, Cin, dw, db, accumulate, s);
}

// dW[co][ci][t] (+)= sum over splits of slab[split][t][co][ci]; db likewise from bslab (may be null)
// The same with the splits shared out over 16 groups of a 1024-thread workgroup (64 outputs per workgroup): the 64- and
// 128-channel layers have one or two output tiles and therefore 100+ splits, which one thread per output walks one dependent
// load after the other (140 us per layer at the very end of the backward pass).  Fixed order: group g sums q = g, g+16, ...,
// the groups are combined in order.
__global__ __launch_bounds__(1024) void wgrad_reduce_wide_f32_kernel(const float* __restrict__ slab, const float* __restrict__ bslab,
                                                                     int splits, int Cout, int Cin, float* __restrict__ dw,
                                                                     float* __restrict__ db, int accumulate) {
  __shared__ float red[16][64];
  const long per = (long)9 * Cout * Cin;
  const long total = per + (bslab ? Cout : 0);
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + c;
  float v = 0.f;
  if (i < per) {
    for (int q = g; q < splits; q += 16) v += slab[(long)q * per + i];
  } else if (i < total) {
    for (int q = g; q < splits; q += 16) v += bslab[(long)q * Cout + (i - per)];
  }
  red[g][c] = v;
  __syncthreads();
  if (g == 0 && i < total) {
    float r = red[0][c];
#pragma unroll
    for (int k = 1; k < 16; ++k) r += red[k][c];
    if (i < per) {
      const int ci = (int)(i % Cin);
      const long rr = i / Cin;
      const int co = (int)(rr % Cout), t = (int)(rr / Cout);
      float* d = dw + ((long)co * Cin + ci) * 9 + t;
      *d = accumulate ? *d + r : r;
    } else {
      const int co = (int)(i - per);
      db[co] = accumulate ? db[co] + r : r;
    }
  }
}

int umpr_wgrad_reduce(const float* slab, const float* bslab, int splits, int Cout, int Cin, float* dw, float* db,
                      int accumulate, hipStream_t s) {
  const long total = (long)9 * Cout * Cin + ((db && bslab) ? Cout : 0);
  if (splits >= 32) {
    wgrad_reduce_wide_f32_kernel<<<(unsigned)((total + 63) / 64), 1024, 0, s>>>(slab, (db && bslab) ? bslab : nullptr, splits,
                                                                              Cout, Cin, dw, db, accumulate);
    UMPR_LAUNCH_CHECK("wgrad_reduce_wide");
    return 0;
  }
  int blocks = (int)((total + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  wgrad_reduce_kernel<<<blocks, 256, 0, s>>>(slab, (db && bslab) ? bslab : nullptr, splits, Cout, Cin, dw, db, accumulate);
  UMPR_LAUNCH_CHECK("wgrad_reduce");
  return 0;
}

int umpr_maxpool2_fwd_impl(const float* x, float* y, long planes, int H, int W, hipStream_t s) {
  UMPR_REQUIRE((H % 2) == 0 && (W % 2) == 0, "maxpool2: odd extent %dx%d", H, W);
  const long total = planes * (H / 2) * (W / 2);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  maxpool2_fwd_kernel<<<blocks, 256, 0, s>>>(x, y, planes, H, W);
  UMPR_LAUNCH_CHECK("maxpool2_fwd");
  return 0;
}

int umpr_maxpool2_bwd_relu_impl(const float* x, const float* gy, float* gx, long planes, int H, int W, hipStream_t s) {
  UMPR_REQUIRE((H % 2) == 0 && (W % 2) == 0, "maxpool2: odd extent %dx%d", H, W);
  const long total = planes * (H / 2) * (W / 2);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  maxpool2_bwd_relu_kernel<<<blocks, 256, 0, s>>>(x, gy, gx, planes, H, W);
  UMPR_LAUNCH_CHECK("maxpool2_bwd_relu");
  return 0;
}
