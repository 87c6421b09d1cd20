// Gradient of the word-embedding table: the scatter of token gradients dx [T][E] into d_emb [vocab][E] (the backward of
// nn.Embedding with freeze=False, src/model.py:237,262-264), deterministic and without atomics.
//
// The caller passes the positions of the (concatenated) token sources stable-sorted by token id (sorted_pos): equal ids then
// form RUNS of consecutive sorted positions, in ascending position order.  The sorted order is cut into WINDOWS of EG_CHUNK
// positions, one wave each (eg_window_kernel): the wave walks its window once, EG_U rows of dx in flight, adding position by
// position and closing a sum wherever the id changes.  A run that lies inside one window is finished there and its table row
// written; a run that crosses a window edge leaves one PIECE per window in the workspace.  The row kernel (eg_rows_kernel) is
// ROW-centric - one wave per 64 consecutive table rows, each lane finds its row's run by binary search - and writes what is left:
// +0.0 for the rows no token names, and for a run of several windows the sum of its pieces in window order.  So
//   * every row of d_emb is written exactly once (no zeroing pass, nobody adds into a row);
//   * a row's sum is chained from +0.0 in one lane per column, in position order inside a piece and in window order over the
//     pieces; where the pieces are cut depends on the sorted ids alone - not on the grid, the scheduling or the device;
//   * the work is balanced by POSITIONS: the pad id and the frequent words (runs of thousands) spread over many waves, and the
//     low, hot rows of a Zipf vocabulary do not queue up in the one wave that owns their 64-row group;
//   * an id outside [0, vocab) is never written: it contributes to no row.
// Three launches: keys (the id behind every sorted position), windows, rows.
//
// umpr_embed_grad_rows keeps the same sums SPARSE (the sparse update of the table, umpr_sparse_adam_rows below): the window walk
// is the same kernel, with a run's sum going to row_grad[j] for the sorted position j at which the run begins instead of to the
// table row, and the finish (eg_finish_kernel) is RUN-centric - the wave of the window in which a run that crosses a window edge
// begins adds its pieces, in the order eg_rows_kernel adds them.  Nothing of size vocab is read or written.
//
// Bound: one pass over the T * E floats of dx and one write of vocab * E floats (80 MB at GloVe-50d, 480 MB at 300d); the keys
// (8 T bytes), the pieces (T * E / 8 bytes) and the binary searches (2 per row, 17 steps at T = 100 k) stay in L2.
#include <math.h>

#include "../../include/umpr_hip.h"
#include "umpr_common.h"
#include "umpr_internal.h"

namespace {

constexpr int EG_CHUNK = 64;       // positions per window = per piece of a long run (umpr_embed_grad_chunk): one per lane
constexpr int EG_MAX_SRC = 4;
constexpr int EG_NB = 5;           // column blocks of 64 a wave carries at once: E <= 320 walks its run once

struct EgSources {
  const int64_t* ids[EG_MAX_SRC];
  const float* dx[EG_MAX_SRC];
  long base[EG_MAX_SRC + 1];       // first concatenated position of source k; T for k >= the number of sources
};

__device__ __forceinline__ int eg_source(const EgSources& S, long pos) {
  int k = 0;
  if (pos >= S.base[1]) k = 1;
  if (pos >= S.base[2]) k = 2;
  if (pos >= S.base[3]) k = 3;
  return k;
}

// keys[j] = the id at sorted position j (a position outside [0, T) - a sorted_pos that is no permutation - names no row)
__global__ __launch_bounds__(256) void eg_keys_kernel(const EgSources S, const int32_t* __restrict__ sorted_pos, long T,
                                                      int64_t* __restrict__ keys) {
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < T; j += (long)gridDim.x * 256) {
    const long pos = sorted_pos[j];
    int64_t key = INT64_MAX;
    if (pos >= 0 && pos < T) {
      const int k = eg_source(S, pos);
      key = S.ids[k][pos - S.base[k]];
    }
    keys[j] = key;
  }
}

__device__ __forceinline__ long eg_lower_bound(const int64_t* __restrict__ keys, long lo, long hi, int64_t v) {
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One wave per window [w EG_CHUNK, (w + 1) EG_CHUNK) of sorted positions.  Lane l holds position w EG_CHUNK + l: its id, its
// source row, and whether a run ends there.  The rows are then loaded U at a time (U independent loads in flight) and added in
// position order; at a run's end the sum goes
//   * to the table row, if the run began in this window (it lies inside it);
//   * to piece 2 w, if the run came in over the window's left edge (it ends here, or - no end at all - covers the window);
// and what is left after the last position - a run that leaves over the right edge - to piece 2 w + 1, or to piece 2 w if that
// run also came in over the left edge.  eg_rows_kernel adds piece 2 w_first + 1 and pieces 2 w for the windows after it.
// ROWS (umpr_embed_grad_rows): `d_emb` is row_grad [T][E] and a run's sum goes to the row of the sorted position at which the run
// begins; row_id [T] and the +0.0 rows of the positions that begin no run of a table row are written here too.
template <int NB, int U, bool ROWS>
__global__ __launch_bounds__(64) void eg_window_kernel(const EgSources S, const int32_t* __restrict__ sorted_pos,
                                                       const int64_t* __restrict__ keys, long T, int E, long vocab,
                                                       float* __restrict__ partial, float* __restrict__ d_emb,
                                                       int64_t* __restrict__ row_id) {
  const int lane = threadIdx.x;
  const long w0 = (long)blockIdx.x * EG_CHUNK;
  const int n = (int)(T - w0 < EG_CHUNK ? T - w0 : EG_CHUNK);
  const long j = w0 + lane;
  int64_t key = -1;
  int pos = -1;
  bool end = false;
  if (lane < n) {
    key = keys[j];
    const int p = sorted_pos[j];
    if (p >= 0 && p < T) pos = p;
    end = j + 1 >= T || keys[j + 1] != key;
  }
  const unsigned long long ends = __ballot(end);
  const bool from_left = w0 > 0 && keys[w0 - 1] == keys[w0];
  const int row_lo = (int)(key & 0xffffffffll), row_hi = (int)(key >> 32);     // the table row of a run, broadcast in two halves
  float* piece = partial + (long)blockIdx.x * 2 * E;
  if constexpr (ROWS) {
    const bool begins = lane < n && key >= 0 && key < vocab && (j == 0 || keys[j - 1] != key);
    if (lane < n) row_id[j] = begins ? key : -1;
    const unsigned long long zero = ~__ballot(begins);  // the window's positions whose row stays +0.0
    float* rows = d_emb + w0 * (long)E;
    for (long idx = lane; idx < (long)n * E; idx += 64)
      if ((zero >> (idx / E)) & 1ull) rows[idx] = 0.f;
  }
  for (int c0 = 0; c0 < E; c0 += 64 * NB) {
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
    bool first = true;                                  // the sum in progress is the window's first
    int begin = 0;                                      // (ROWS) where in the window it began
    for (int i = 0; i < n; i += U) {                    // i + u <= 63: U divides 64
      float x[U][NB];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int p = __shfl(pos, i + u, 64);           // -1 past the end of the window and for a position outside [0, T): adds +0.0
        const bool ok = p >= 0;
        const long pp = ok ? p : 0;
        const int k = eg_source(S, pp);
        const float* r = S.dx[k] + (pp - S.base[k]) * (long)E;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const int c = c0 + 64 * b + lane;
          x[u][b] = (ok && c < E) ? r[c] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] += x[u][b];
        if ((ends >> (i + u)) & 1ull) {                 // wave-uniform
          float* dst = nullptr;
          if (first && from_left) {
            dst = piece;
          } else {
            const long row = ((long)__shfl(row_hi, i + u, 64) << 32) | (unsigned int)__shfl(row_lo, i + u, 64);
            if (row >= 0 && row < vocab) dst = d_emb + (ROWS ? w0 + begin : row) * (long)E;
          }
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const int c = c0 + 64 * b + lane;
            if (dst && c < E) dst[c] = acc[b];
            acc[b] = 0.f;
          }
          first = false;
          begin = i + u + 1;
        }
      }
    }
    if (!((ends >> (n - 1)) & 1ull)) {                  // the last run leaves over the right edge
      float* dst = piece + ((first && from_left) ? 0 : E);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int c = c0 + 64 * b + lane;
        if (c < E) dst[c] = acc[b];
      }
    }
  }
}

// dst [E] = the sum of the pieces of a run that begins in window wf and ends in window wl > wf: piece 2 wf + 1, then pieces 2 w in
// window order, eight loads in flight (one wave, a lane per column)
template <int NB>
__device__ __forceinline__ void eg_add_pieces(const float* __restrict__ partial, int wf, int wl, int E, int lane,
                                              float* __restrict__ dst) {
  for (int c0 = 0; c0 < E; c0 += 64 * NB) {
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
    for (int w0 = wf; w0 <= wl; w0 += 8) {
      float x[8][NB];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int w = w0 + u;
        const bool ok = w <= wl;
        const float* src = partial + (2 * (long)(ok ? w : wf) + (w == wf ? 1 : 0)) * E;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const int c = c0 + 64 * b + lane;
          x[u][b] = (ok && c < E) ? src[c] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] += x[u][b];
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int c = c0 + 64 * b + lane;
      if (c < E) dst[c] = acc[b];
    }
  }
}

// One wave per group of 64 consecutive table rows: lane l finds the run of row r0 + l, the wave zero-fills the untouched rows of
// the group - as one contiguous span of 16-byte stores when no row of the group is touched and the table is 16-byte aligned,
// row by row otherwise - leaves the rows whose run lies inside one window to eg_window_kernel, which wrote them, and adds the
// pieces of the runs that cross a window edge.
template <int NB>
__global__ __launch_bounds__(256) void eg_rows_kernel(const int64_t* __restrict__ keys, int T, int E, long vocab,
                                                      const float* __restrict__ partial, float* __restrict__ d_emb) {
  const int lane = threadIdx.x & 63;
  const long groups = (vocab + 63) / 64;
  const bool aligned = ((uintptr_t)d_emb & 15u) == 0;
  for (long grp = (long)blockIdx.x * 4 + (threadIdx.x >> 6); grp < groups; grp += (long)gridDim.x * 4) {
    const long r0 = grp * 64;
    const int nrows = (int)(vocab - r0 < 64 ? vocab - r0 : 64);
    const long v = r0 + lane;
    int lo = 0, hi = 0;
    if (lane < nrows && T > 0) {
      lo = (int)eg_lower_bound(keys, 0, T, v);
      if (lo < T && keys[lo] == v) hi = (int)eg_lower_bound(keys, lo + 1, T, v + 1);
    }
    const unsigned long long mask = __ballot(hi > lo);
    float* span = d_emb + r0 * (long)E;
    const long n = (long)nrows * E;
    if (mask == 0 && aligned) {                       // r0 * E * 4 bytes is a multiple of 256: the span starts 16-byte aligned
      const long n4 = n >> 2;
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      for (long i = lane; i < n4; i += 64) reinterpret_cast<float4*>(span)[i] = z;
      const long i = 4 * n4 + lane;
      if (i < n) span[i] = 0.f;
      continue;
    }
    for (int r = 0; r < nrows; ++r) {                 // row by row (wave-uniform): zeros, or the sum of the row's run
      float* dst = span + (long)r * E;
      if (!((mask >> r) & 1ull)) {
        for (int c = lane; c < E; c += 64) dst[c] = 0.f;
        continue;
      }
      const int rlo = __shfl(lo, r, 64), rhi = __shfl(hi, r, 64);
      const int wf = rlo / EG_CHUNK, wl = (rhi - 1) / EG_CHUNK;
      if (wf == wl) continue;                          // inside one window: written there
      eg_add_pieces<NB>(partial, wf, wl, E, lane, dst);
    }
  }
}

// (umpr_embed_grad_rows) One wave per window: if a run of a table row BEGINS in this window and leaves it over the right edge, the
// wave finds the run's end (one binary search, from the window's edge on) and writes the sum of its pieces - in eg_rows_kernel's
// order - to the row of the position at which the run begins.  Every other wave has nothing to do.
template <int NB>
__global__ __launch_bounds__(256) void eg_finish_kernel(const int64_t* __restrict__ keys, long T, int E, long vocab,
                                                        const float* __restrict__ partial, float* __restrict__ row_grad) {
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long w0 = w * EG_CHUNK, next = w0 + EG_CHUNK;
  if (next >= T) return;                                // the last window (or none): its last run ends with it
  const int64_t key = keys[next - 1];
  if (keys[next] != key || key < 0 || key >= vocab) return;
  const unsigned long long same = __ballot(keys[w0 + lane] == key);     // sorted: the run's positions are the top lanes
  if (same == ~0ull && w0 > 0 && keys[w0 - 1] == key) return;           // the run came in over the left edge: not this wave's
  const long begin = w0 + __ffsll(same) - 1;
  const long end = eg_lower_bound(keys, next, T, key + 1);
  eg_add_pieces<NB>(partial, (int)w, (int)((end - 1) / EG_CHUNK), E, lane, row_grad + begin * (long)E);
}

// Row-wise Adam in torch.optim.SparseAdam's form on the rows umpr_embed_grad_rows left: one wave per window of sorted positions,
// and for each row_id[j] >= 0 of the window that wave alone reads and writes row row_id[j] of p, m and v (a lane per column, NB
// column blocks at once).  A table row is owned by the one position at which its run begins, so no two waves meet.
template <int NB>
__global__ __launch_bounds__(256) void sparse_adam_rows_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                               long vocab, int E, const int64_t* __restrict__ row_id,
                                                               const float* __restrict__ row_grad, long T, float gscale0, float b1,
                                                               float b2, float eps, float step_size,
                                                               const float* __restrict__ state) {
  float gscale = gscale0;
  if (state != nullptr) {
    if (state[UMPR_CLIP_FINITE] == 0.f) return;
    gscale = gscale0 * state[UMPR_CLIP_COEF];
  }
  const int lane = threadIdx.x & 63;
  const long w0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * EG_CHUNK;
  if (w0 >= T) return;
  const long j = w0 + lane;
  const int64_t id = j < T ? row_id[j] : -1;
  const int row_lo = (int)(id & 0xffffffffll), row_hi = (int)(id >> 32);
  unsigned long long todo = __ballot(id >= 0 && id < vocab);
  while (todo) {                                        // wave-uniform
    const int i = __ffsll(todo) - 1;
    todo &= todo - 1;
    const long row = ((long)__shfl(row_hi, i, 64) << 32) | (unsigned int)__shfl(row_lo, i, 64);
    const float* __restrict__ g = row_grad + (w0 + i) * (long)E;
    const long at = row * (long)E;
    for (int c0 = 0; c0 < E; c0 += 64 * NB) {
      float gi[NB], pi[NB], mi[NB], vi[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int c = c0 + 64 * b + lane;
        const bool ok = c < E;
        gi[b] = ok ? g[c] : 0.f;
        pi[b] = ok ? p[at + c] : 0.f;
        mi[b] = ok ? m[at + c] : 0.f;
        vi[b] = ok ? v[at + c] : 0.f;
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int c = c0 + 64 * b + lane;
        const float gs = gi[b] * gscale;
        const float mn = b1 * mi[b] + (1.f - b1) * gs;
        const float vn = b2 * vi[b] + (1.f - b2) * gs * gs;
        if (c < E) {
          m[at + c] = mn;
          v[at + c] = vn;
          p[at + c] = pi[b] - step_size * (mn / (sqrtf(vn) + eps));
        }
      }
    }
  }
}

inline size_t eg_keys_bytes(long T) { return align_up((size_t)T * sizeof(int64_t), 256); }
inline long eg_windows(long T) { return (T + EG_CHUNK - 1) / EG_CHUNK; }
constexpr long EG_MAX_T = 2147483647L - 2 * EG_CHUNK;   // sorted_pos is int32

// the source table of umpr_embed_grad / umpr_embed_grad_rows, checked; T = the number of tokens
int eg_sources(const char* who, const int64_t* const* ids, const float* const* dx, const long* counts, int n_src,
               const int32_t* sorted_pos, EgSources& S, long& T) {
  UMPR_REQUIRE(n_src >= 0 && n_src <= EG_MAX_SRC, "%s: %d sources outside 0..%d", who, n_src, EG_MAX_SRC);
  UMPR_REQUIRE(n_src == 0 || (ids != nullptr && dx != nullptr && counts != nullptr), "%s: null source table", who);
  T = 0;
  for (int k = 0; k < EG_MAX_SRC; ++k) {
    const long n = k < n_src ? counts[k] : 0;
    UMPR_REQUIRE(n >= 0 && n <= EG_MAX_T - T, "%s: source %d: bad count %ld", who, k, n);
    UMPR_REQUIRE(n == 0 || (ids[k] != nullptr && dx[k] != nullptr), "%s: source %d: null ids / dx", who, k);
    S.ids[k] = n > 0 ? ids[k] : nullptr;
    S.dx[k] = n > 0 ? dx[k] : nullptr;
    S.base[k] = T;
    T += n;
  }
  S.base[EG_MAX_SRC] = T;
  for (int k = n_src; k < EG_MAX_SRC; ++k) S.base[k] = T;
  UMPR_REQUIRE(T == 0 || sorted_pos != nullptr, "%s: sorted_pos is NULL", who);
  return 0;
}

}  // namespace

extern "C" {

int umpr_embed_grad_chunk(void) { return EG_CHUNK; }

size_t umpr_embed_grad_ws_bytes(long T, int E) {
  if (T <= 0 || E <= 0) return 0;
  return eg_keys_bytes(T) + align_up((size_t)(2 * eg_windows(T)) * E * sizeof(float), 256);
}

int umpr_embed_grad(const int64_t* const* ids, const float* const* dx, const long* counts, int n_src, int E, long vocab,
                    const int32_t* sorted_pos, float* d_emb, void* ws, size_t ws_bytes, void* stream) {
  UMPR_REQUIRE(E >= 1 && vocab >= 1 && d_emb != nullptr, "embed_grad: bad E=%d / vocab=%ld / d_emb", E, vocab);
  EgSources S;
  long T = 0;
  if (int rc = eg_sources("embed_grad", ids, dx, counts, n_src, sorted_pos, S, T)) return rc;
  UMPR_REQUIRE(ws_bytes >= umpr_embed_grad_ws_bytes(T, E) && (T == 0 || ws != nullptr), "embed_grad: workspace too small");
  UMPR_REQUIRE(((uintptr_t)ws & 7u) == 0, "embed_grad: the workspace must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int64_t* keys = static_cast<int64_t*>(ws);
  float* partial = T > 0 ? reinterpret_cast<float*>(static_cast<char*>(ws) + eg_keys_bytes(T)) : nullptr;
  if (T > 0) {
    long kb = (T + 255) / 256;
    if (kb > 4096) kb = 4096;
    eg_keys_kernel<<<(unsigned)kb, 256, 0, s>>>(S, sorted_pos, T, keys);
    UMPR_LAUNCH_CHECK("embed_grad keys");
    const unsigned wn = (unsigned)eg_windows(T);
    if (E <= 64) eg_window_kernel<1, 16, false><<<wn, 64, 0, s>>>(S, sorted_pos, keys, T, E, vocab, partial, d_emb, nullptr);
    else eg_window_kernel<EG_NB, 8, false><<<wn, 64, 0, s>>>(S, sorted_pos, keys, T, E, vocab, partial, d_emb, nullptr);
    UMPR_LAUNCH_CHECK("embed_grad windows");
  }
  long rb = ((vocab + 63) / 64 + 3) / 4;
  if (rb > 8192) rb = 8192;
  if (E <= 64) eg_rows_kernel<1><<<(unsigned)rb, 256, 0, s>>>(keys, (int)T, E, vocab, partial, d_emb);
  else eg_rows_kernel<EG_NB><<<(unsigned)rb, 256, 0, s>>>(keys, (int)T, E, vocab, partial, d_emb);
  UMPR_LAUNCH_CHECK("embed_grad rows");
  return 0;
}

size_t umpr_embed_grad_rows_ws_bytes(long T, int E) { return umpr_embed_grad_ws_bytes(T, E); }

int umpr_embed_grad_rows(const int64_t* const* ids, const float* const* dx, const long* counts, int n_src, int E, long vocab,
                         const int32_t* sorted_pos, int64_t* row_id, float* row_grad, void* ws, size_t ws_bytes, void* stream) {
  UMPR_REQUIRE(E >= 1 && vocab >= 1, "embed_grad_rows: bad E=%d / vocab=%ld", E, vocab);
  EgSources S;
  long T = 0;
  if (int rc = eg_sources("embed_grad_rows", ids, dx, counts, n_src, sorted_pos, S, T)) return rc;
  if (T == 0) return 0;
  UMPR_REQUIRE(row_id != nullptr && row_grad != nullptr, "embed_grad_rows: row_id / row_grad is NULL");
  UMPR_REQUIRE(ws_bytes >= umpr_embed_grad_rows_ws_bytes(T, E) && ws != nullptr, "embed_grad_rows: workspace too small");
  UMPR_REQUIRE(((uintptr_t)ws & 7u) == 0, "embed_grad_rows: the workspace must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int64_t* keys = static_cast<int64_t*>(ws);
  float* partial = reinterpret_cast<float*>(static_cast<char*>(ws) + eg_keys_bytes(T));
  long kb = (T + 255) / 256;
  if (kb > 4096) kb = 4096;
  eg_keys_kernel<<<(unsigned)kb, 256, 0, s>>>(S, sorted_pos, T, keys);
  UMPR_LAUNCH_CHECK("embed_grad_rows keys");
  const unsigned wn = (unsigned)eg_windows(T);
  if (E <= 64) eg_window_kernel<1, 16, true><<<wn, 64, 0, s>>>(S, sorted_pos, keys, T, E, vocab, partial, row_grad, row_id);
  else eg_window_kernel<EG_NB, 8, true><<<wn, 64, 0, s>>>(S, sorted_pos, keys, T, E, vocab, partial, row_grad, row_id);
  UMPR_LAUNCH_CHECK("embed_grad_rows windows");
  if (wn > 1) {                                         // a run can cross an edge only where there is one
    if (E <= 64) eg_finish_kernel<1><<<(wn + 3) / 4, 256, 0, s>>>(keys, T, E, vocab, partial, row_grad);
    else eg_finish_kernel<EG_NB><<<(wn + 3) / 4, 256, 0, s>>>(keys, T, E, vocab, partial, row_grad);
    UMPR_LAUNCH_CHECK("embed_grad_rows finish");
  }
  return 0;
}

int umpr_sparse_adam_rows(float* p, float* m, float* v, long vocab, int E, const int64_t* row_id, const float* row_grad, long T,
                          double lr, double beta1, double beta2, double eps, long step, double grad_scale,
                          const float* clip_state, void* stream) {
  UMPR_REQUIRE(E >= 1 && vocab >= 1 && step >= 1 && T >= 0, "sparse_adam_rows: bad E=%d / vocab=%ld / step=%ld / T=%ld", E, vocab,
               step, T);
  if (T == 0) return 0;
  UMPR_REQUIRE(p != nullptr && m != nullptr && v != nullptr && row_id != nullptr && row_grad != nullptr,
               "sparse_adam_rows: null p / m / v / row_id / row_grad");
  UMPR_REQUIRE(T <= EG_MAX_T, "sparse_adam_rows: bad T=%ld", T);
  // torch.optim.SparseAdam: step_size = lr * sqrt(1 - beta2^t) / (1 - beta1^t), eps added to sqrt(v) itself
  const double step_size = lr * sqrt(1.0 - pow(beta2, (double)step)) / (1.0 - pow(beta1, (double)step));
  const unsigned blocks = (unsigned)((eg_windows(T) + 3) / 4);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (E <= 64)
    sparse_adam_rows_kernel<1><<<blocks, 256, 0, s>>>(p, m, v, vocab, E, row_id, row_grad, T, (float)grad_scale, (float)beta1,
                                                      (float)beta2, (float)eps, (float)step_size, clip_state);
  else
    sparse_adam_rows_kernel<EG_NB><<<blocks, 256, 0, s>>>(p, m, v, vocab, E, row_id, row_grad, T, (float)grad_scale, (float)beta1,
                                                          (float)beta2, (float)eps, (float)step_size, clip_state);
  UMPR_LAUNCH_CHECK("sparse_adam_rows");
  return 0;
}

}  // extern "C"
