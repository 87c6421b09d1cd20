// Gradient clipping by global norm inside the optimiser step: one deterministic 2-norm over the flat gradient arenas and the two
// Adam kernels of text_ops.hip with the clip coefficient read from device memory (umpr_amd/optim.py::FusedAdam(max_grad_norm=)).
// And the sum of the gradient arenas over the micro-batches of one optimiser step (FusedAdam.accumulate, --accum_steps).
#include <math.h>

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

// adam_kernel / adam_dev_kernel (text_ops.hip) with the gradient scale multiplied by the clip coefficient - ONE float product of
// the two scalars, so that coef == 1 leaves the scale, and with it every bit of the update, as the unclipped kernels have it.  A
// step whose gradient norm was not finite touches nothing.
__global__ void adam_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                 float* __restrict__ v, long n, float gscale0, float wd, float b1, float b2, float eps,
                                 float step_size, float inv_bc2_sqrt, const float* __restrict__ state) {
  if (state[UMPR_CLIP_FINITE] == 0.f) return;
  const float gscale = gscale0 * state[UMPR_CLIP_COEF];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float pi = p[i];
    const float gi = g[i] * gscale + wd * pi;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) * inv_bc2_sqrt + eps;
    p[i] = pi - step_size * (mi / denom);
  }
}

__global__ void adam_dev_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                     float* __restrict__ v, long n, float b1, float b2, float eps,
                                     const float* __restrict__ hyper, const float* __restrict__ state) {
  if (state[UMPR_CLIP_FINITE] == 0.f) return;
  const float gscale = hyper[0] * state[UMPR_CLIP_COEF], step_size = hyper[1], inv_bc2_sqrt = hyper[2], wd = hyper[3];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float pi = p[i];
    const float gi = g[i] * gscale + wd * pi;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) * inv_bc2_sqrt + eps;
    p[i] = pi - step_size * (mi / denom);
  }
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

inline int adam_blocks(long n) {      // the grid of umpr_adam_impl / umpr_adam_dev_impl
  long b = (n + 255) / 256;
  return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
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

int umpr_adam_step_clip(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                        double eps, double weight_decay, long step, double grad_scale, const float* state, void* stream) {
  UMPR_REQUIRE(step >= 1 && n >= 0 && state != nullptr, "adam_clip: bad step/n/state");
  if (n == 0) return 0;
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const double step_size = lr / bc1;
  const double inv_bc2_sqrt = 1.0 / sqrt(bc2);
  adam_clip_kernel<<<adam_blocks(n), 256, 0, S(stream)>>>(p, g, m, v, n, (float)grad_scale, (float)weight_decay, (float)beta1,
                                                          (float)beta2, (float)eps, (float)step_size, (float)inv_bc2_sqrt, state);
  UMPR_LAUNCH_CHECK("adam_clip");
  return 0;
}

int umpr_adam_step_dev_clip(float* p, const float* g, float* m, float* v, long n, double beta1, double beta2, double eps,
                            const float* hyper, const float* state, void* stream) {
  UMPR_REQUIRE(n >= 0 && hyper != nullptr && state != nullptr, "adam_dev_clip: bad arguments");
  if (n == 0) return 0;
  adam_dev_clip_kernel<<<adam_blocks(n), 256, 0, S(stream)>>>(p, g, m, v, n, (float)beta1, (float)beta2, (float)eps, hyper,
                                                              state);
  UMPR_LAUNCH_CHECK("adam_dev_clip");
  return 0;
}

}  // extern "C"
