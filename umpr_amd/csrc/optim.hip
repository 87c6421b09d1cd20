// The optimiser's kernels on the flat arenas (umpr_amd/optim.py::FusedAdam).  The dense Adam update: ONE element function, ONE
// kernel template <DEV, CLIP> and ONE launcher behind the four entry points umpr_adam_step[_dev][_clip] - per-step scalars by
// value or from device memory (graph mode), without or with the clip coefficient read from device memory - so that the four
// forms are bit-identical at coefficient 1 by construction.  The template's two further switches <SEG, DECOUPLED> - a table of up
// to 16 segments with their own learning-rate and decay multipliers in one launch, and AdamW's decoupled decay - sit behind a
// fifth entry point, umpr_adam_step_groups (FusedAdam(lr_scales=, wd_scales=, decoupled_decay=)).  Gradient clipping by global norm (FusedAdam(max_grad_norm=)): one
// deterministic 2-norm over the gradient arenas.  And the sum of the gradient arenas over the micro-batches of one optimiser
// step (FusedAdam.accumulate, --accum_steps).  And the exponential moving average of the parameter arenas (FusedAdam(ema_decay=),
// --ema_decay) with the exchange of two sets of arenas that puts the average under the model for an evaluation.
#include <math.h>

#include <type_traits>

#include "../../include/umpr_hip.h"
#include "umpr_common.h"
#include "umpr_internal.h"

namespace {

// The grid of stage one is FIXED: it depends neither on the element count nor on the device, so that every element is always
// summed by the same thread in the same position of the same chain and the result is a pure function of the bytes (every rank of
// a data-parallel job gets the same coefficient from the same all-reduced arena).  2048 workgroups = 8 per CU on 256 CUs.
constexpr int GN_BLOCKS = 2048, GN_THREADS = 256, GN_MAX_ARENAS = 8;
constexpr long GN_SWEEP = (long)GN_BLOCKS * GN_THREADS;   // float4s one pass of the grid covers

struct GradArenas {
  const float* p[GN_MAX_ARENAS];
  long n[GN_MAX_ARENAS];
  int count;
};

__device__ __forceinline__ double sq_acc(double acc, float x) {
  const double d = (double)x;          // a 24-bit significand squared has 48 bits: the product is exact in double,
  return fma(d, d, acc);               // and the fused add rounds once - the sum of exact squares, chained per thread
}
__device__ __forceinline__ double sq_acc4(double acc, const float4 q) {
  return sq_acc(sq_acc(sq_acc(sq_acc(acc, q.x), q.y), q.z), q.w);
}

// 256 threads -> one double in thread 0: shuffle tree per wave, then the four waves in order (sq_err_accumulate_kernel's tree)
__device__ __forceinline__ double block_sum_256(double s, double* part) {
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}

// Stage one.  Per arena: up to three scalar elements in front of the first 16-byte boundary, float4s in grid-stride order (four
// independent loads and four independent chains per thread while at least four passes remain, then one per pass), up to three
// scalar elements behind the last whole float4.  One double per workgroup.
__global__ void __launch_bounds__(GN_THREADS) grad_sq_partial_kernel(const GradArenas A, double* __restrict__ partial) {
  __shared__ double part[4];
  const long gid = (long)blockIdx.x * GN_THREADS + threadIdx.x;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int a = 0; a < A.count; ++a) {
    const float* __restrict__ g = A.p[a];
    const long n = A.n[a];
    if (n <= 0) continue;
    long head = (long)(((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    const long n4 = (n - head) >> 2;
    const long tail0 = head + 4 * n4;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + head);
    long i = gid;
    for (; i + 3 * GN_SWEEP < n4; i += 4 * GN_SWEEP) {
      const float4 q0 = g4[i], q1 = g4[i + GN_SWEEP], q2 = g4[i + 2 * GN_SWEEP], q3 = g4[i + 3 * GN_SWEEP];
      s0 = sq_acc4(s0, q0); s1 = sq_acc4(s1, q1); s2 = sq_acc4(s2, q2); s3 = sq_acc4(s3, q3);
    }
    for (; i < n4; i += GN_SWEEP) s0 = sq_acc4(s0, g4[i]);
    if (gid < head) s1 = sq_acc(s1, g[gid]);
    if (gid < n - tail0) s2 = sq_acc(s2, g[tail0 + gid]);
  }
  const double s = block_sum_256((s0 + s1) + (s2 + s3), part);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Stage two: one workgroup adds the 2048 partials in a fixed order (eight consecutive ones per thread, then the tree) and thread 0
// writes the state.  torch.nn.utils.clip_grad_norm_: coef = min(1, max_norm / (norm + 1e-6)), here in double, rounded once.
__global__ void __launch_bounds__(GN_THREADS) grad_norm_finish_kernel(const double* __restrict__ partial, double max_norm,
                                                                      float gscale, const float* __restrict__ gscale_dev,
                                                                      float* __restrict__ state) {
  __shared__ double part[4];
  constexpr int PER = GN_BLOCKS / GN_THREADS;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < PER; ++k) s += partial[threadIdx.x * PER + k];
  const double sum = block_sum_256(s, part);
  if (threadIdx.x != 0) return;
  const float gs = gscale_dev ? gscale_dev[0] : gscale;
  const double norm = sqrt(sum) * fabs((double)gs);
  const bool finite = isfinite(sum) && isfinite(norm);
  const float coef = finite ? (float)fmin(1.0, max_norm / (norm + 1e-6)) : 0.f;
  uint32_t* cnt = reinterpret_cast<uint32_t*>(state);
  state[UMPR_CLIP_COEF] = coef;
  state[UMPR_CLIP_NORM] = (float)norm;
  state[UMPR_CLIP_FINITE] = finite ? 1.f : 0.f;
  state[UMPR_CLIP_MAX_NORM] = (float)max_norm;
  cnt[UMPR_CLIP_SEEN] += 1u;
  if (!finite) cnt[UMPR_CLIP_SKIPPED] += 1u;
  else if (coef < 1.f) cnt[UMPR_CLIP_CLIPPED] += 1u;
}

// Adam with coupled L2 exactly as torch.optim.Adam applies it (main.py:22-25), for one element:
//   g += wd*p; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// in floats:  gi = g*gscale + wd*p;  mi = b1*m + (1-b1)*gi;  vi = b2*v + (1-b2)*gi*gi;  denom = sqrtf(vi)*inv_bc2_sqrt + eps;
//             p - step_size*(mi/denom)
// Which product of `a*b + c*d` goes into the fma is the compiler's choice, and with the kernel's scalars in another argument
// order it chose the other one: left to it, two instantiations of the template below differed in the last bit of gi.  So the
// fusions are written out - the ones every build of this update has made so far (profiles/r14_a_adam_unify.txt) - and
// contraction is off for the rest: the bits are the source's, whatever the instantiation.
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float gscale, float wd, float b1, float b2,
                                            float eps, float step_size, float inv_bc2_sqrt) {
#pragma clang fp contract(off)
  const float pi = p;
  const float gi = fmaf(wd, pi, g * gscale);
  const float mi = fmaf(1.f - b1, gi, b1 * m);
  const float vi = b2 * v + (1.f - b2) * gi * gi;
  m = mi; v = vi;
  const float denom = fmaf(sqrtf(vi), inv_bc2_sqrt, eps);
  p = fmaf(-step_size, mi / denom, pi);
}

// AdamW's decoupled decay (FusedAdam(decoupled_decay=True), torch.optim.AdamW) for one element: the parameter shrinks first, the
// gradient carries no decay term:
//   p *= 1 - lr*wd; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// in floats:  pi = p*keep, keep = 1 - decay, decay = lr*wd (one float per segment);  gi = g*gscale;  mi = b1*m + (1-b1)*gi;
//             vi = b2*v + (1-b2)*gi*gi;  denom = sqrtf(vi)*inv_bc2_sqrt + eps;  pi - step_size*(mi/denom)
// The same fusions as adam_update, written out, contraction off.
__device__ __forceinline__ void adamw_update(float& p, float g, float& m, float& v, float gscale, float keep, float b1, float b2,
                                             float eps, float step_size, float inv_bc2_sqrt) {
#pragma clang fp contract(off)
  const float pi = p * keep;
  const float gi = g * gscale;
  const float mi = fmaf(1.f - b1, gi, b1 * m);
  const float vi = b2 * v + (1.f - b2) * gi * gi;
  m = mi; v = vi;
  const float denom = fmaf(sqrtf(vi), inv_bc2_sqrt, eps);
  p = fmaf(-step_size, mi / denom, pi);
}

// Where one launch gets its per-step scalars.  By value from the host, or (DEV) from device memory: hyper[0..3] = grad_scale,
// step_size = lr / (1 - b1^t), 1 / sqrt(1 - b2^t), weight_decay as the caller will use them for the NEXT launch - what a captured
// hipGraph of a training step launches: the node's kernel arguments are frozen at capture, the bias corrections change every
// step.  CLIP adds the 8-float state umpr_grad_norm left; the forms without it carry an empty struct in the pointer's place.
// In the decoupled form the fourth scalar is lr * weight_decay, the fraction a parameter with multipliers 1 shrinks by.
struct AdamScalars { float gscale, step_size, inv_bc2_sqrt, wd; };
struct NoClipState {};

// The segments of one launch (FusedAdam(lr_scales=, wd_scales=)): elements [end[k-1], end[k]) of the launch - end[-1] = 0 - take
// step_size * lr_mult[k] and wd * wd_mult[k], ONE float product each, so that multipliers of exactly 1 leave every bit of the
// update as the plain forms have it.  Every end but the last is a multiple of 64 elements, so the 64 consecutive elements one
// wave handles in one pass of the grid (256-thread blocks, a grid stride that is a multiple of 256) lie in one segment whatever
// the base pointers' alignment: the lookup is wave-uniform, and the table holds the ends in WAVES, end / 64, as 32-bit numbers -
// the scalar unit compares those, it has no 64-bit less-than.  The last end, n, and every entry behind it are ceil(n / 64), which
// no wave's number reaches; those entries repeat the last multipliers.  The table travels in the kernel arguments, as GradArenas
// does.
constexpr int ADAM_MAX_SEGS = 16, ADAM_THREADS = 256;
struct AdamSegs {
  unsigned end_wave[ADAM_MAX_SEGS];
  float lr_mult[ADAM_MAX_SEGS];
  float wd_mult[ADAM_MAX_SEGS];
};
struct NoSegs {};

// One step of the lookup: a wave at or behind `end` takes the next segment's multipliers.  All six operands are wave-uniform.
// Written as the scalar unit's compare and two selects: left to the compiler, the chain of selects between floats became 30
// vector selects per element (it keeps floats in vector registers), and a count of the ends in front of the wave a vector
// population count - on a kernel whose vector unit has the update itself to do.
__device__ __forceinline__ void seg_pick(float& lr_mult, float& wd_mult, unsigned wave, unsigned end, float lr_next,
                                         float wd_next) {
  asm("s_cmp_ge_u32 %2, %3\n\ts_cselect_b32 %0, %4, %0\n\ts_cselect_b32 %1, %5, %1"
      : "+s"(lr_mult), "+s"(wd_mult)
      : "s"(wave), "s"(end), "s"(lr_next), "s"(wd_next)
      : "scc");
}

// The one dense Adam kernel.  CLIP: a step whose gradient norm was not finite touches nothing - the decoupled shrink included -
// and the gradient scale is multiplied by the clip coefficient - ONE float product of the two scalars, so that coef == 1 leaves
// the scale, and with it every bit of the update, as the forms without CLIP have it.  SEG: per-segment multipliers, looked up
// once per wave and pass from the wave's first element - a value every lane agrees on and the compiler is told so
// (readfirstlane of the wave's number), which keeps the comparisons and both selected multipliers in scalar registers.
// DECOUPLED: adamw_update in place of adam_update.
template <bool DEV, bool CLIP, bool SEG, bool DECOUPLED>
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            long n, float b1, float b2, float eps, std::conditional_t<DEV, const float*, AdamScalars> hyper,
                            std::conditional_t<CLIP, const float*, NoClipState> state,
                            const std::conditional_t<SEG, AdamSegs, NoSegs> segs) {
#pragma clang fp contract(off)
  static_assert(SEG || !DECOUPLED, "the decoupled form always carries a segment table (one segment when nothing is scaled)");
  if constexpr (CLIP) {
    if (state[UMPR_CLIP_FINITE] == 0.f) return;
  }
  AdamScalars a;
  if constexpr (DEV) a = AdamScalars{hyper[0], hyper[1], hyper[2], hyper[3]};
  else a = hyper;
  if constexpr (CLIP) a.gscale = a.gscale * state[UMPR_CLIP_COEF];
  const long stride = (long)gridDim.x * blockDim.x;
  if constexpr (!SEG) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride)
      adam_update(p[i], g[i], m[i], v[i], a.gscale, a.wd, b1, b2, eps, a.step_size, a.inv_bc2_sqrt);
  } else {
    // the number of this wave's 64 elements among the launch's: the same in every lane, and the compiler is told so
    unsigned wave = blockIdx.x * (ADAM_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned wave_stride = gridDim.x * (ADAM_THREADS / 64);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride, wave += wave_stride) {
      float lr_mult = segs.lr_mult[0], wd_mult = segs.wd_mult[0];
#pragma unroll
      for (int k = 1; k < ADAM_MAX_SEGS; ++k)
        seg_pick(lr_mult, wd_mult, wave, segs.end_wave[k - 1], segs.lr_mult[k], segs.wd_mult[k]);
      const float step_size = a.step_size * lr_mult, wd = a.wd * wd_mult;
      if constexpr (DECOUPLED) adamw_update(p[i], g[i], m[i], v[i], a.gscale, 1.f - wd, b1, b2, eps, step_size, a.inv_bc2_sqrt);
      else adam_update(p[i], g[i], m[i], v[i], a.gscale, wd, b1, b2, eps, step_size, a.inv_bc2_sqrt);
    }
  }
}

// 256 threads, min(ceil(n / 256), 8192) workgroups (n >= 1 here), grid-stride loop: a second pass of the grid from 8192 * 256
// elements on.  Elementwise, so the grid has no say in the result.
template <bool DEV, bool CLIP, bool SEG = false, bool DECOUPLED = false, class Hyper, class State, class Segs = NoSegs>
int adam_launch(const char* what, float* p, const float* g, float* m, float* v, long n, double b1, double b2, double eps,
                Hyper hyper, State state, void* stream, Segs segs = Segs{}) {
  if (n == 0) return 0;
  const long blocks = (n + ADAM_THREADS - 1) / ADAM_THREADS;
  adam_kernel<DEV, CLIP, SEG, DECOUPLED>
      <<<(int)(blocks > 8192 ? 8192 : blocks), ADAM_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
          p, g, m, v, n, (float)b1, (float)b2, (float)eps, hyper, state, segs);
  UMPR_LAUNCH_CHECK(what);
  return 0;
}

// The host forms' bias corrections, in double as torch computes them, rounded to float once.
AdamScalars adam_host_scalars(double lr, double beta1, double beta2, double weight_decay, long step, double grad_scale) {
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const double step_size = lr / bc1;
  const double inv_bc2_sqrt = 1.0 / sqrt(bc2);
  return AdamScalars{(float)grad_scale, (float)step_size, (float)inv_bc2_sqrt, (float)weight_decay};
}

// Gradient accumulation over micro-batches (FusedAdam.accumulate): acc = g (FIRST: acc is never read, so whatever it holds - the
// NaN or inf of a skipped step included - costs no zeroing pass) or acc += g, one fp32 add per element.  A pure HBM stream of 8
// or 12 bytes per element on the fixed grid of the norm kernel above; elementwise, so the grid has no say in the result.  Per
// arena: scalar elements in front of the first 16-byte boundary, float4s in grid-stride order (four independent loads per
// stream and thread while at least four passes remain), scalar elements behind the last whole float4.  Where the two bases
// sit differently inside a 16-byte line no float4 fits both, and the arena goes element by element.
constexpr int GA_BLOCKS = GN_BLOCKS, GA_THREADS = GN_THREADS, GA_MAX_ARENAS = GN_MAX_ARENAS;
constexpr long GA_SWEEP = (long)GA_BLOCKS * GA_THREADS;   // float4s (or, on the scalar path, floats) one pass of the grid covers

struct AccArenas {
  float* acc[GA_MAX_ARENAS];
  const float* g[GA_MAX_ARENAS];
  long n[GA_MAX_ARENAS];
  int count;
};

template <bool FIRST>
__device__ __forceinline__ float acc1(float a, float g) { return FIRST ? g : a + g; }
template <bool FIRST>
__device__ __forceinline__ float4 acc4(const float4 a, const float4 g) {
  return FIRST ? g : make_float4(a.x + g.x, a.y + g.y, a.z + g.z, a.w + g.w);
}

template <bool FIRST>
__global__ void __launch_bounds__(GA_THREADS) grad_accumulate_kernel(const AccArenas A) {
  const long gid = (long)blockIdx.x * GA_THREADS + threadIdx.x;
  const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int a = 0; a < A.count; ++a) {
    float* __restrict__ acc = A.acc[a];
    const float* __restrict__ g = A.g[a];
    const long n = A.n[a];
    if (n <= 0) continue;
    if ((((uintptr_t)acc ^ (uintptr_t)g) & 15u) != 0) {
      for (long i = gid; i < n; i += GA_SWEEP) acc[i] = acc1<FIRST>(FIRST ? 0.f : acc[i], g[i]);
      continue;
    }
    long head = (long)(((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    const long n4 = (n - head) >> 2;
    const long tail0 = head + 4 * n4;
    float4* __restrict__ acc_4 = reinterpret_cast<float4*>(acc + head);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + head);
    long i = gid;
    for (; i + 3 * GA_SWEEP < n4; i += 4 * GA_SWEEP) {
      const float4 q0 = g4[i], q1 = g4[i + GA_SWEEP], q2 = g4[i + 2 * GA_SWEEP], q3 = g4[i + 3 * GA_SWEEP];
      const float4 a0 = FIRST ? none : acc_4[i], a1 = FIRST ? none : acc_4[i + GA_SWEEP];
      const float4 a2 = FIRST ? none : acc_4[i + 2 * GA_SWEEP], a3 = FIRST ? none : acc_4[i + 3 * GA_SWEEP];
      acc_4[i] = acc4<FIRST>(a0, q0);
      acc_4[i + GA_SWEEP] = acc4<FIRST>(a1, q1);
      acc_4[i + 2 * GA_SWEEP] = acc4<FIRST>(a2, q2);
      acc_4[i + 3 * GA_SWEEP] = acc4<FIRST>(a3, q3);
    }
    for (; i < n4; i += GA_SWEEP) acc_4[i] = acc4<FIRST>(FIRST ? none : acc_4[i], g4[i]);
    if (gid < head) acc[gid] = acc1<FIRST>(FIRST ? 0.f : acc[gid], g[gid]);
    if (gid < n - tail0) acc[tail0 + gid] = acc1<FIRST>(FIRST ? 0.f : acc[tail0 + gid], g[tail0 + gid]);
  }
}

// Exponential moving average of the parameters (FusedAdam(ema_decay=)): ema = p (FIRST: ema is never read, so it needs no
// initialising pass, whatever it holds) or ema += w * (p - ema), w = 1 - decay, on the grid and with the access pattern of
// grad_accumulate_kernel above (AccArenas: acc is the average, g the parameters).  8 or 12 bytes per element.  The subtraction
// is rounded to float, then ONE fused multiply-add: what torch.lerp(ema, p, w) computes on the CPU for w < 0.5.  Written out
// with contraction off, as adam_update is: the bits are the source's.
__device__ __forceinline__ float ema1(float e, float p, float w) {
#pragma clang fp contract(off)
  const float d = p - e;
  return fmaf(w, d, e);
}
template <bool FIRST>
__device__ __forceinline__ float4 ema4(const float4 e, const float4 p, float w) {
  return FIRST ? p : make_float4(ema1(e.x, p.x, w), ema1(e.y, p.y, w), ema1(e.z, p.z, w), ema1(e.w, p.w, w));
}

template <bool FIRST>
__global__ void __launch_bounds__(GA_THREADS) ema_update_kernel(const AccArenas A, float w) {
  const long gid = (long)blockIdx.x * GA_THREADS + threadIdx.x;
  const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int a = 0; a < A.count; ++a) {
    float* __restrict__ ema = A.acc[a];
    const float* __restrict__ p = A.g[a];
    const long n = A.n[a];
    if (n <= 0) continue;
    if ((((uintptr_t)ema ^ (uintptr_t)p) & 15u) != 0) {
      for (long i = gid; i < n; i += GA_SWEEP) ema[i] = FIRST ? p[i] : ema1(ema[i], p[i], w);
      continue;
    }
    long head = (long)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    const long n4 = (n - head) >> 2;
    const long tail0 = head + 4 * n4;
    float4* __restrict__ ema_4 = reinterpret_cast<float4*>(ema + head);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + head);
    long i = gid;
    for (; i + 3 * GA_SWEEP < n4; i += 4 * GA_SWEEP) {
      const float4 q0 = p4[i], q1 = p4[i + GA_SWEEP], q2 = p4[i + 2 * GA_SWEEP], q3 = p4[i + 3 * GA_SWEEP];
      const float4 e0 = FIRST ? none : ema_4[i], e1 = FIRST ? none : ema_4[i + GA_SWEEP];
      const float4 e2 = FIRST ? none : ema_4[i + 2 * GA_SWEEP], e3 = FIRST ? none : ema_4[i + 3 * GA_SWEEP];
      ema_4[i] = ema4<FIRST>(e0, q0, w);
      ema_4[i + GA_SWEEP] = ema4<FIRST>(e1, q1, w);
      ema_4[i + 2 * GA_SWEEP] = ema4<FIRST>(e2, q2, w);
      ema_4[i + 3 * GA_SWEEP] = ema4<FIRST>(e3, q3, w);
    }
    for (; i < n4; i += GA_SWEEP) ema_4[i] = ema4<FIRST>(FIRST ? none : ema_4[i], p4[i], w);
    if (gid < head) ema[gid] = FIRST ? p[gid] : ema1(ema[gid], p[gid], w);
    if (gid < n - tail0) ema[tail0 + gid] = FIRST ? p[tail0 + gid] : ema1(ema[tail0 + gid], p[tail0 + gid], w);
  }
}

// The exchange of two sets of arenas (FusedAdam.swapped_ema): a[k] <-> b[k], moves only, so every bit travels - NaN payloads,
// signed zeros, infinities.  16 bytes per element, the same grid and access pattern; a[k] and b[k] do not overlap (refused by
// the entry point), so every element is read and written by one thread only.
struct SwapArenas {
  float* a[GA_MAX_ARENAS];
  float* b[GA_MAX_ARENAS];
  long n[GA_MAX_ARENAS];
  int count;
};

__global__ void __launch_bounds__(GA_THREADS) arena_swap_kernel(const SwapArenas A) {
  const long gid = (long)blockIdx.x * GA_THREADS + threadIdx.x;
  for (int k = 0; k < A.count; ++k) {
    float* __restrict__ a = A.a[k];
    float* __restrict__ b = A.b[k];
    const long n = A.n[k];
    if (n <= 0) continue;
    if ((((uintptr_t)a ^ (uintptr_t)b) & 15u) != 0) {
      for (long i = gid; i < n; i += GA_SWEEP) {
        const float x = a[i], y = b[i];
        a[i] = y; b[i] = x;
      }
      continue;
    }
    long head = (long)(((16u - (unsigned)((uintptr_t)a & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    const long n4 = (n - head) >> 2;
    const long tail0 = head + 4 * n4;
    float4* __restrict__ a4 = reinterpret_cast<float4*>(a + head);
    float4* __restrict__ b4 = reinterpret_cast<float4*>(b + head);
    long i = gid;
    for (; i + 3 * GA_SWEEP < n4; i += 4 * GA_SWEEP) {
      const float4 x0 = a4[i], x1 = a4[i + GA_SWEEP], x2 = a4[i + 2 * GA_SWEEP], x3 = a4[i + 3 * GA_SWEEP];
      const float4 y0 = b4[i], y1 = b4[i + GA_SWEEP], y2 = b4[i + 2 * GA_SWEEP], y3 = b4[i + 3 * GA_SWEEP];
      a4[i] = y0; a4[i + GA_SWEEP] = y1; a4[i + 2 * GA_SWEEP] = y2; a4[i + 3 * GA_SWEEP] = y3;
      b4[i] = x0; b4[i + GA_SWEEP] = x1; b4[i + 2 * GA_SWEEP] = x2; b4[i + 3 * GA_SWEEP] = x3;
    }
    for (; i < n4; i += GA_SWEEP) {
      const float4 x = a4[i], y = b4[i];
      a4[i] = y; b4[i] = x;
    }
    if (gid < head) {
      const float x = a[gid], y = b[gid];
      a[gid] = y; b[gid] = x;
    }
    if (gid < n - tail0) {
      const float x = a[tail0 + gid], y = b[tail0 + gid];
      a[tail0 + gid] = y; b[tail0 + gid] = x;
    }
  }
}

inline hipStream_t S(void* s) { return static_cast<hipStream_t>(s); }

}  // namespace

extern "C" {

size_t umpr_grad_norm_ws_bytes(void) { return (size_t)GN_BLOCKS * sizeof(double); }

int umpr_grad_norm(const float* const* grads, const long* counts, int n_arenas, double max_norm, float grad_scale,
                   const float* grad_scale_dev, double* ws, size_t ws_bytes, float* state, void* stream) {
  UMPR_REQUIRE(n_arenas >= 0 && n_arenas <= GN_MAX_ARENAS, "grad_norm: %d arenas outside 0..%d", n_arenas, GN_MAX_ARENAS);
  UMPR_REQUIRE(n_arenas == 0 || (grads != nullptr && counts != nullptr), "grad_norm: null arena table");
  UMPR_REQUIRE(ws != nullptr && state != nullptr && ws_bytes >= umpr_grad_norm_ws_bytes(), "grad_norm: workspace too small");
  UMPR_REQUIRE(max_norm >= 0.0 && isfinite(max_norm), "grad_norm: max_norm must be finite and not negative");
  GradArenas A;
  A.count = n_arenas;
  for (int a = 0; a < GN_MAX_ARENAS; ++a) {
    A.p[a] = a < n_arenas ? grads[a] : nullptr;
    A.n[a] = a < n_arenas ? counts[a] : 0;
    UMPR_REQUIRE(A.n[a] >= 0 && (A.n[a] == 0 || A.p[a] != nullptr), "grad_norm: arena %d: bad pointer / count", a);
    UMPR_REQUIRE(((uintptr_t)A.p[a] & 3u) == 0, "grad_norm: arena %d is not aligned to a float", a);
  }
  grad_sq_partial_kernel<<<GN_BLOCKS, GN_THREADS, 0, S(stream)>>>(A, ws);
  UMPR_LAUNCH_CHECK("grad_norm stage 1");
  grad_norm_finish_kernel<<<1, GN_THREADS, 0, S(stream)>>>(ws, max_norm, grad_scale, grad_scale_dev, state);
  UMPR_LAUNCH_CHECK("grad_norm stage 2");
  return 0;
}

int umpr_grad_accumulate(float* const* acc, const float* const* grads, const long* counts, int n_arenas, int first,
                         void* stream) {
  UMPR_REQUIRE(n_arenas >= 0 && n_arenas <= GA_MAX_ARENAS, "grad_accumulate: %d arenas outside 0..%d", n_arenas, GA_MAX_ARENAS);
  UMPR_REQUIRE(n_arenas == 0 || (acc != nullptr && grads != nullptr && counts != nullptr), "grad_accumulate: null arena table");
  AccArenas A;
  A.count = n_arenas;
  long total = 0;
  for (int a = 0; a < GA_MAX_ARENAS; ++a) {
    A.acc[a] = a < n_arenas ? acc[a] : nullptr;
    A.g[a] = a < n_arenas ? grads[a] : nullptr;
    A.n[a] = a < n_arenas ? counts[a] : 0;
    UMPR_REQUIRE(A.n[a] >= 0 && (A.n[a] == 0 || (A.acc[a] != nullptr && A.g[a] != nullptr)),
                 "grad_accumulate: arena %d: bad pointer / count", a);
    UMPR_REQUIRE((((uintptr_t)A.acc[a] | (uintptr_t)A.g[a]) & 3u) == 0, "grad_accumulate: arena %d is not aligned to a float", a);
    total += A.n[a];
  }
  if (total == 0) return 0;
  if (first) grad_accumulate_kernel<true><<<GA_BLOCKS, GA_THREADS, 0, S(stream)>>>(A);
  else grad_accumulate_kernel<false><<<GA_BLOCKS, GA_THREADS, 0, S(stream)>>>(A);
  UMPR_LAUNCH_CHECK("grad_accumulate");
  return 0;
}

int umpr_ema_update(float* const* ema, const float* const* params, const long* counts, int n_arenas, double decay, int first,
                    void* stream) {
  UMPR_REQUIRE(n_arenas >= 0 && n_arenas <= GA_MAX_ARENAS, "ema_update: %d arenas outside 0..%d", n_arenas, GA_MAX_ARENAS);
  UMPR_REQUIRE(n_arenas == 0 || (ema != nullptr && params != nullptr && counts != nullptr), "ema_update: null arena table");
  UMPR_REQUIRE(decay > 0.5 && decay < 1.0, "ema_update: decay %g outside the open interval (0.5, 1)", decay);
  AccArenas A;
  A.count = n_arenas;
  long total = 0;
  for (int a = 0; a < GA_MAX_ARENAS; ++a) {
    A.acc[a] = a < n_arenas ? ema[a] : nullptr;
    A.g[a] = a < n_arenas ? params[a] : nullptr;
    A.n[a] = a < n_arenas ? counts[a] : 0;
    UMPR_REQUIRE(A.n[a] >= 0 && (A.n[a] == 0 || (A.acc[a] != nullptr && A.g[a] != nullptr)),
                 "ema_update: arena %d: bad pointer / count", a);
    UMPR_REQUIRE((((uintptr_t)A.acc[a] | (uintptr_t)A.g[a]) & 3u) == 0, "ema_update: arena %d is not aligned to a float", a);
    total += A.n[a];
  }
  if (total == 0) return 0;
  const float w = (float)(1.0 - decay);
  if (first) ema_update_kernel<true><<<GA_BLOCKS, GA_THREADS, 0, S(stream)>>>(A, w);
  else ema_update_kernel<false><<<GA_BLOCKS, GA_THREADS, 0, S(stream)>>>(A, w);
  UMPR_LAUNCH_CHECK("ema_update");
  return 0;
}

int umpr_arena_swap(float* const* a, float* const* b, const long* counts, int n_arenas, void* stream) {
  UMPR_REQUIRE(n_arenas >= 0 && n_arenas <= GA_MAX_ARENAS, "arena_swap: %d arenas outside 0..%d", n_arenas, GA_MAX_ARENAS);
  UMPR_REQUIRE(n_arenas == 0 || (a != nullptr && b != nullptr && counts != nullptr), "arena_swap: null arena table");
  SwapArenas A;
  A.count = n_arenas;
  long total = 0;
  for (int k = 0; k < GA_MAX_ARENAS; ++k) {
    A.a[k] = k < n_arenas ? a[k] : nullptr;
    A.b[k] = k < n_arenas ? b[k] : nullptr;
    A.n[k] = k < n_arenas ? counts[k] : 0;
    UMPR_REQUIRE(A.n[k] >= 0 && (A.n[k] == 0 || (A.a[k] != nullptr && A.b[k] != nullptr)),
                 "arena_swap: arena %d: bad pointer / count", k);
    UMPR_REQUIRE((((uintptr_t)A.a[k] | (uintptr_t)A.b[k]) & 3u) == 0, "arena_swap: arena %d is not aligned to a float", k);
    const uintptr_t lo_a = (uintptr_t)A.a[k], lo_b = (uintptr_t)A.b[k], bytes = (uintptr_t)A.n[k] * sizeof(float);
    UMPR_REQUIRE(A.n[k] == 0 || lo_a + bytes <= lo_b || lo_b + bytes <= lo_a, "arena_swap: arena %d: the two ranges overlap", k);
    total += A.n[k];
  }
  if (total == 0) return 0;
  arena_swap_kernel<<<GA_BLOCKS, GA_THREADS, 0, S(stream)>>>(A);
  UMPR_LAUNCH_CHECK("arena_swap");
  return 0;
}

int umpr_adam_step(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                   double eps, double weight_decay, long step, double grad_scale, void* stream) {
  UMPR_REQUIRE(step >= 1 && n >= 0, "adam: bad step/n");
  return adam_launch<false, false>("adam", p, g, m, v, n, beta1, beta2, eps,
                                   adam_host_scalars(lr, beta1, beta2, weight_decay, step, grad_scale), NoClipState{}, stream);
}

int umpr_adam_step_dev(float* p, const float* g, float* m, float* v, long n, double beta1, double beta2, double eps,
                       const float* hyper, void* stream) {
  UMPR_REQUIRE(n >= 0 && hyper != nullptr, "adam_dev: bad arguments");
  return adam_launch<true, false>("adam_dev", p, g, m, v, n, beta1, beta2, eps, hyper, NoClipState{}, stream);
}

int umpr_adam_step_clip(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                        double eps, double weight_decay, long step, double grad_scale, const float* state, void* stream) {
  UMPR_REQUIRE(step >= 1 && n >= 0 && state != nullptr, "adam_clip: bad step/n/state");
  return adam_launch<false, true>("adam_clip", p, g, m, v, n, beta1, beta2, eps,
                                  adam_host_scalars(lr, beta1, beta2, weight_decay, step, grad_scale), state, stream);
}

int umpr_adam_step_dev_clip(float* p, const float* g, float* m, float* v, long n, double beta1, double beta2, double eps,
                            const float* hyper, const float* state, void* stream) {
  UMPR_REQUIRE(n >= 0 && hyper != nullptr && state != nullptr, "adam_dev_clip: bad arguments");
  return adam_launch<true, true>("adam_dev_clip", p, g, m, v, n, beta1, beta2, eps, hyper, state, stream);
}

int umpr_adam_step_groups(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                          double eps, double weight_decay, long step, double grad_scale, const float* hyper,
                          const float* clip_state, const long* seg_end, const float* seg_lr_mult, const float* seg_wd_mult,
                          int n_segs, int decoupled, void* stream) {
  UMPR_REQUIRE(n >= 0 && (hyper != nullptr || step >= 1), "adam_groups: bad step/n");
  if (n == 0) return 0;
  UMPR_REQUIRE((n + 63) / 64 <= 0xffffffffL, "adam_groups: n = %ld: more than 2^32 waves of 64 elements", n);
  UMPR_REQUIRE(n_segs >= 1 && n_segs <= ADAM_MAX_SEGS, "adam_groups: %d segments outside 1..%d", n_segs, ADAM_MAX_SEGS);
  UMPR_REQUIRE(seg_end != nullptr && seg_lr_mult != nullptr && seg_wd_mult != nullptr, "adam_groups: null segment table");
  AdamSegs segs;
  long prev = 0;
  for (int k = 0; k < n_segs; ++k) {
    const long end = seg_end[k];
    const float a = seg_lr_mult[k], w = seg_wd_mult[k];
    UMPR_REQUIRE(end > prev && end <= n, "adam_groups: segment %d ends at %ld: not behind %ld or past n = %ld", k, end, prev, n);
    UMPR_REQUIRE(k == n_segs - 1 || end % 64 == 0, "adam_groups: segment %d ends at %ld, not a multiple of 64 elements", k, end);
    UMPR_REQUIRE(k < n_segs - 1 || end == n, "adam_groups: the last segment ends at %ld, not at n = %ld", end, n);
    UMPR_REQUIRE(isfinite(a) && a > 0.f, "adam_groups: segment %d: learning-rate multiplier %g is not finite and > 0", k, (double)a);
    UMPR_REQUIRE(isfinite(w) && w >= 0.f, "adam_groups: segment %d: decay multiplier %g is not finite and >= 0", k, (double)w);
    // decoupled: the segment shrinks by (lr * a) * (wd * w): its one multiplier of the launch's lr * wd is a * w, rounded once
    segs.end_wave[k] = (unsigned)((end + 63) / 64);
    segs.lr_mult[k] = a;
    segs.wd_mult[k] = decoupled ? (float)((double)a * (double)w) : w;
    prev = end;
  }
  for (int k = n_segs; k < ADAM_MAX_SEGS; ++k) {      // never selected: no wave's number reaches ceil(n / 64)
    segs.end_wave[k] = segs.end_wave[n_segs - 1];
    segs.lr_mult[k] = segs.lr_mult[n_segs - 1];
    segs.wd_mult[k] = segs.wd_mult[n_segs - 1];
  }
  // the decoupled forms' fourth scalar: lr * weight_decay, rounded to float once (FusedAdam.hyper_rows makes the same double)
  AdamScalars host{};
  if (hyper == nullptr) {
    host = adam_host_scalars(lr, beta1, beta2, weight_decay, step, grad_scale);
    if (decoupled) host.wd = (float)(lr * weight_decay);
  }
  const char* what = "adam_groups";
#define UMPR_ADAM_GROUPS(DEC)                                                                                                    \
  (hyper != nullptr                                                                                                              \
       ? (clip_state != nullptr                                                                                                  \
              ? adam_launch<true, true, true, DEC>(what, p, g, m, v, n, beta1, beta2, eps, hyper, clip_state, stream, segs)        \
              : adam_launch<true, false, true, DEC>(what, p, g, m, v, n, beta1, beta2, eps, hyper, NoClipState{}, stream, segs))   \
       : (clip_state != nullptr                                                                                                  \
              ? adam_launch<false, true, true, DEC>(what, p, g, m, v, n, beta1, beta2, eps, host, clip_state, stream, segs)        \
              : adam_launch<false, false, true, DEC>(what, p, g, m, v, n, beta1, beta2, eps, host, NoClipState{}, stream, segs)))
  return decoupled ? UMPR_ADAM_GROUPS(true) : UMPR_ADAM_GROUPS(false);
#undef UMPR_ADAM_GROUPS
}

}  // extern "C"
