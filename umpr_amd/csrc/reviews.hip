// Review collate on the GPU: the tokenised sentences of a corpus are a constant of the run, so umpr_amd/reviews.py::ReviewStore
// keeps them in device memory - every distinct sentence once in a token arena, and per role (user, item, ui) a CSR table from
// sample to sentence ids - and a batch travels as B sample indices.  This kernel finishes umpr_amd/data.py::batch_loader's text
// half: it writes the padded [2][B][S][L] user+item ids (the two halves of the one allocation UMPR.forward takes as ids_pair),
// the [B][S_ui][L_ui] ui ids and the [B] labels, bit for bit what pad_reviews + torch.LongTensor give on the host.
//
// The indices are read on the host (the caller passes them in host memory) and validated against n_samples, then travel in the
// kernel arguments, kIdxChunk per launch: no index can make the kernel read outside the tables, and the launch needs no
// hipMemcpy (capture-safe).  The tables themselves live in device memory; the kernel clips what it reads from them to the
// output's shape and to n_sent, so a corrupt table gives wrong ids, never an out-of-bounds write.
#include "umpr_common.h"
#include "../../include/umpr_hip.h"

namespace {

constexpr int kIdxChunk = 256;    // 256 x 4 B of kernel arguments per launch: a batch of up to 256 samples is ONE launch
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxLen = 256;      // the model's max_sent_length bound

struct IdxChunk {
  int32_t n[kIdxChunk];
};

struct Role {
  const int64_t* ptr;   // [n_samples + 1]
  const int32_t* sid;   // [nnz]
};

// One wave per output row (role, s) of one sample, lanes along l: a wave's stores are 64 consecutive int64.  blockIdx.y = sample
// of the chunk (its index is a wave-uniform kernel-argument load), blockIdx.x * kWaves + wave = row: the S user rows, the S item
// rows, then the S_ui ui rows.  Every element of every row is written exactly once - the token or `pad`.
__global__ __launch_bounds__(kThreads) void review_collate_kernel(IdxChunk chunk, int first, int B, int S, int L, int S_ui, int L_ui,
                                                                  long pad, const int32_t* __restrict__ tokens,
                                                                  const int64_t* __restrict__ sent_off, long n_sent, Role ru, Role ri,
                                                                  Role rui, const float* __restrict__ ratings,
                                                                  int64_t* __restrict__ ids_pair, int64_t* __restrict__ ids_ui,
                                                                  float* __restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int b = first + blockIdx.y;
  const long n = chunk.n[blockIdx.y];
  if (blockIdx.x == 0 && threadIdx.x == 0) labels[b] = ratings[n];
  if (row >= 2 * S + S_ui) return;
  Role r;
  int s, len_cap;
  int64_t* out;
  if (row < 2 * S) {
    const int half = row >= S;
    r = half ? ri : ru;
    s = row - half * S;
    len_cap = L;
    out = ids_pair + (((size_t)half * B + b) * S + s) * L;
  } else {
    r = rui;
    s = row - 2 * S;
    len_cap = L_ui;
    out = ids_ui + ((size_t)b * S_ui + s) * L_ui;
  }
  const int64_t p0 = r.ptr[n];
  const int64_t count = r.ptr[n + 1] - p0;
  const int32_t* src = nullptr;
  int len = 0;
  if (s < count) {
    const long j = r.sid[p0 + s];
    if (j >= 0 && j < n_sent) {
      const int64_t o = sent_off[j];
      const int64_t m = sent_off[j + 1] - o;
      src = tokens + o;
      len = (int)(m < 0 ? 0 : m > len_cap ? len_cap : m);
    }
  }
  for (int l = lane; l < len_cap; l += 64) out[l] = l < len ? (int64_t)src[l] : (int64_t)pad;
}

// ---- sampled collate (umpr_amd/reviews.py::ReviewDraw) --------------------------------------------------------------------------------
// The same rows, but which sentences of a user's or an item's pool fill them is drawn anew per (seed, epoch, sample, role), and
// tokens may be replaced by `unk`.  Counter-based: every number is splitmix64's output function of a key the host definition
// (reviews.py::ReviewTable.draw) forms the same way, so the kernel holds no state and agrees with it bit for bit.
constexpr int kMaxPool = 1024;    // sentences of one pool the ranking looks at: the LDS key table's size
constexpr int kPerThread = kMaxPool / kThreads;
constexpr uint64_t kDropKey = 0xD6E8FEB86659FD93ull;   // separates the dropout stream from the sentence keys of the same role

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// One workgroup per (sample of the chunk, role): blockIdx.y = sample, blockIdx.x = role (user, item, ui).  For user and item the
// block hashes a key per pool position into LDS, ranks every key by counting the keys below it (ties to the smaller position) and
// leaves the sentence id of rank s < keep in slot[s]; then its waves write the role's rows as review_collate_kernel does, one
// wave per row, lanes along l, every element of every row exactly once.  The ui role writes its sentences in table order.
template <bool kDrop>
__global__ __launch_bounds__(kThreads) void review_collate_sampled_kernel(
    IdxChunk chunk, int first, int B, int S, int L, int S_ui, int L_ui, long pad, const int32_t* __restrict__ tokens,
    const int64_t* __restrict__ sent_off, long n_sent, Role ru, Role ri, Role rui, const float* __restrict__ ratings,
    int64_t* __restrict__ ids_pair, int64_t* __restrict__ ids_ui, float* __restrict__ labels, int keep, uint64_t seed_epoch_key,
    uint32_t drop_threshold, long unk) {
  __shared__ uint64_t keys[kMaxPool];
  __shared__ int32_t slot[kMaxPool];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int role = blockIdx.x;
  const int b = first + blockIdx.y;
  const long n = chunk.n[blockIdx.y];
  if (role == 0 && tid == 0) labels[b] = ratings[n];
  const int rows = role < 2 ? S : S_ui;
  if (rows <= 0) return;                                         // (block-uniform: no ui output)
  const Role r = role == 0 ? ru : role == 1 ? ri : rui;
  const int len_cap = role < 2 ? L : L_ui;
  int64_t* const out0 = role < 2 ? ids_pair + ((size_t)role * B + b) * S * L : ids_ui + (size_t)b * S_ui * L_ui;
  const int64_t p0 = r.ptr[n];
  const int64_t cnt = r.ptr[n + 1] - p0;
  const uint64_t role_key = mix64(mix64(seed_epoch_key + (uint64_t)n) + (uint64_t)role);
  int valid;                                                     // rows that hold a sentence
  if (role < 2) {
    const int n_pool = (int)(cnt < 0 ? 0 : cnt > kMaxPool ? kMaxPool : cnt);
    // a thread owns the positions tid + q * kThreads: their keys stay in registers, and one pass over the LDS table ranks them all
    uint64_t mine[kPerThread];
    int rank[kPerThread];
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
      const int j = tid + q * kThreads;
      mine[q] = mix64(role_key + (uint64_t)j);
      rank[q] = 0;
      if (j < n_pool) keys[j] = mine[q];
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < n_pool; ++i) {
      const uint64_t ki = keys[i];                               // the same address in every lane: an LDS broadcast
#pragma unroll
      for (int q = 0; q < kPerThread; ++q) rank[q] += (ki < mine[q]) | ((ki == mine[q]) & (i < tid + q * kThreads));
    }
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
      const int j = tid + q * kThreads;                          // the ranks are a permutation of 0 .. n_pool - 1; keep <= kMaxPool
      if (j < n_pool && rank[q] < keep) slot[rank[q]] = r.sid[p0 + j];
    }
    __syncthreads();
    valid = n_pool < keep ? n_pool : keep;
  } else {
    valid = (int)(cnt < 0 ? 0 : cnt > rows ? rows : cnt);
  }
  const uint64_t drop_key = mix64(role_key ^ kDropKey);
  for (int s = tid >> 6; s < rows; s += kWaves) {
    const int32_t* src = nullptr;
    int len = 0;
    if (s < valid) {
      const long j = role < 2 ? slot[s] : r.sid[p0 + s];
      if (j >= 0 && j < n_sent) {
        const int64_t o = sent_off[j];
        const int64_t m = sent_off[j + 1] - o;
        src = tokens + o;
        len = (int)(m < 0 ? 0 : m > len_cap ? len_cap : m);
      }
    }
    int64_t* const out = out0 + (size_t)s * len_cap;
    for (int l = lane; l < len_cap; l += 64) {
      int64_t v = (int64_t)pad;
      if (l < len) {
        v = (int64_t)src[l];
        if (kDrop) {
          const uint64_t h = mix64(drop_key + (((uint64_t)s << 8) | (uint64_t)l));
          if ((uint32_t)(h >> 32) < drop_threshold) v = (int64_t)unk;
        }
      }
      out[l] = v;
    }
  }
}

}  // namespace

extern "C" int umpr_review_collate(const int32_t* tokens, const int64_t* sent_off, long n_sent, const int64_t* ptr_u,
                                   const int32_t* sid_u, const int64_t* ptr_i, const int32_t* sid_i, const int64_t* ptr_ui,
                                   const int32_t* sid_ui, const float* ratings, long n_samples, const int32_t* idx, int B, int S, int L,
                                   int S_ui, int L_ui, long pad, int64_t* ids_pair, int64_t* ids_ui, float* labels, void* stream) {
  UMPR_REQUIRE(tokens != nullptr, "review_collate: null tokens");
  UMPR_REQUIRE(sent_off != nullptr, "review_collate: null sent_off");
  UMPR_REQUIRE(idx != nullptr, "review_collate: null idx");
  UMPR_REQUIRE(ids_pair != nullptr, "review_collate: null ids_pair");
  UMPR_REQUIRE(labels != nullptr, "review_collate: null labels");
  UMPR_REQUIRE(ratings != nullptr, "review_collate: null ratings");
  UMPR_REQUIRE(ptr_u != nullptr && sid_u != nullptr, "review_collate: null table of the user role");
  UMPR_REQUIRE(ptr_i != nullptr && sid_i != nullptr, "review_collate: null table of the item role");
  UMPR_REQUIRE(B >= 1, "review_collate: B = %d", B);
  UMPR_REQUIRE(n_sent >= 0 && n_samples >= 0, "review_collate: n_sent = %ld, n_samples = %ld", n_sent, n_samples);
  UMPR_REQUIRE(S >= 1 && L >= 1 && L <= kMaxLen, "review_collate: bad shape S = %d, L = %d (S >= 1, 1 <= L <= %d)", S, L, kMaxLen);
  if (ids_ui == nullptr) {
    UMPR_REQUIRE(S_ui == 0 && L_ui == 0, "review_collate: null ids_ui with S_ui = %d, L_ui = %d (both must be 0)", S_ui, L_ui);
  } else {
    UMPR_REQUIRE(S_ui >= 1 && L_ui >= 1 && L_ui <= kMaxLen,
                 "review_collate: ids_ui given with S_ui = %d, L_ui = %d (S_ui >= 1, 1 <= L_ui <= %d)", S_ui, L_ui, kMaxLen);
    UMPR_REQUIRE(ptr_ui != nullptr && sid_ui != nullptr, "review_collate: null table of the ui role");
  }
  UMPR_REQUIRE((long)S <= (1L << 20) && (long)S_ui <= (1L << 20), "review_collate: S = %d, S_ui = %d above 2^20", S, S_ui);
  UMPR_REQUIRE(((uintptr_t)ids_pair & 7) == 0 && ((uintptr_t)ids_ui & 7) == 0 && ((uintptr_t)sent_off & 7) == 0 &&
                   ((uintptr_t)ptr_u & 7) == 0 && ((uintptr_t)ptr_i & 7) == 0 && ((uintptr_t)ptr_ui & 7) == 0,
               "review_collate: an int64 array is not 8-byte aligned");
  for (int i = 0; i < B; ++i)
    UMPR_REQUIRE(idx[i] >= 0 && idx[i] < n_samples, "review_collate: index %d of the batch is %d, outside the %ld samples", i, idx[i],
                 n_samples);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int rows = 2 * S + S_ui;
  for (int first = 0; first < B; first += kIdxChunk) {
    const int cnt = min(kIdxChunk, B - first);
    IdxChunk chunk = {};
    memcpy(chunk.n, idx + first, sizeof(int32_t) * cnt);
    review_collate_kernel<<<dim3(cdiv(rows, kWaves), cnt), kThreads, 0, s>>>(chunk, first, B, S, L, S_ui, L_ui, pad, tokens, sent_off,
                                                                              n_sent, Role{ptr_u, sid_u}, Role{ptr_i, sid_i},
                                                                              Role{ptr_ui, sid_ui}, ratings, ids_pair, ids_ui, labels);
    UMPR_LAUNCH_CHECK("review_collate");
  }
  return 0;
}

extern "C" int umpr_review_collate_sampled(const int32_t* tokens, const int64_t* sent_off, long n_sent, const int64_t* ptr_u,
                                           const int32_t* sid_u, const int64_t* ptr_i, const int32_t* sid_i, const int64_t* ptr_ui,
                                           const int32_t* sid_ui, const float* ratings, long n_samples, const int32_t* idx, int B,
                                           int S, int L, int S_ui, int L_ui, long pad, int keep, uint64_t seed_epoch_key,
                                           unsigned int drop_threshold, long unk, int64_t* ids_pair, int64_t* ids_ui, float* labels,
                                           void* stream) {
  UMPR_REQUIRE(tokens != nullptr, "review_collate_sampled: null tokens");
  UMPR_REQUIRE(sent_off != nullptr, "review_collate_sampled: null sent_off");
  UMPR_REQUIRE(idx != nullptr, "review_collate_sampled: null idx");
  UMPR_REQUIRE(ids_pair != nullptr, "review_collate_sampled: null ids_pair");
  UMPR_REQUIRE(labels != nullptr, "review_collate_sampled: null labels");
  UMPR_REQUIRE(ratings != nullptr, "review_collate_sampled: null ratings");
  UMPR_REQUIRE(ptr_u != nullptr && sid_u != nullptr, "review_collate_sampled: null table of the user role");
  UMPR_REQUIRE(ptr_i != nullptr && sid_i != nullptr, "review_collate_sampled: null table of the item role");
  UMPR_REQUIRE(B >= 1, "review_collate_sampled: B = %d", B);
  UMPR_REQUIRE(n_sent >= 0 && n_samples >= 0, "review_collate_sampled: n_sent = %ld, n_samples = %ld", n_sent, n_samples);
  UMPR_REQUIRE(S >= 1 && L >= 1 && L <= kMaxLen, "review_collate_sampled: bad shape S = %d, L = %d (S >= 1, 1 <= L <= %d)", S, L,
               kMaxLen);
  if (ids_ui == nullptr) {
    UMPR_REQUIRE(S_ui == 0 && L_ui == 0, "review_collate_sampled: null ids_ui with S_ui = %d, L_ui = %d (both must be 0)", S_ui,
                 L_ui);
  } else {
    UMPR_REQUIRE(S_ui >= 1 && L_ui >= 1 && L_ui <= kMaxLen,
                 "review_collate_sampled: ids_ui given with S_ui = %d, L_ui = %d (S_ui >= 1, 1 <= L_ui <= %d)", S_ui, L_ui, kMaxLen);
    UMPR_REQUIRE(ptr_ui != nullptr && sid_ui != nullptr, "review_collate_sampled: null table of the ui role");
  }
  UMPR_REQUIRE((long)S <= (1L << 20) && (long)S_ui <= (1L << 20), "review_collate_sampled: S = %d, S_ui = %d above 2^20", S, S_ui);
  UMPR_REQUIRE(((uintptr_t)ids_pair & 7) == 0 && ((uintptr_t)ids_ui & 7) == 0 && ((uintptr_t)sent_off & 7) == 0 &&
                   ((uintptr_t)ptr_u & 7) == 0 && ((uintptr_t)ptr_i & 7) == 0 && ((uintptr_t)ptr_ui & 7) == 0,
               "review_collate_sampled: an int64 array is not 8-byte aligned");
  UMPR_REQUIRE(keep >= 1 && keep <= kMaxPool, "review_collate_sampled: keep = %d (1 <= keep <= %d)", keep, kMaxPool);
  UMPR_REQUIRE(S <= keep, "review_collate_sampled: S = %d rows above keep = %d", S, keep);
  UMPR_REQUIRE(drop_threshold == 0 || unk >= 0, "review_collate_sampled: a drop threshold of %u without an unk id (unk = %ld)",
               drop_threshold, unk);
  for (int i = 0; i < B; ++i)
    UMPR_REQUIRE(idx[i] >= 0 && idx[i] < n_samples, "review_collate_sampled: index %d of the batch is %d, outside the %ld samples",
                 i, idx[i], n_samples);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  for (int first = 0; first < B; first += kIdxChunk) {
    const int cnt = min(kIdxChunk, B - first);
    IdxChunk chunk = {};
    memcpy(chunk.n, idx + first, sizeof(int32_t) * cnt);
    const dim3 grid(3, cnt);
    if (drop_threshold != 0)
      review_collate_sampled_kernel<true><<<grid, kThreads, 0, s>>>(chunk, first, B, S, L, S_ui, L_ui, pad, tokens, sent_off, n_sent,
                                                                    Role{ptr_u, sid_u}, Role{ptr_i, sid_i}, Role{ptr_ui, sid_ui},
                                                                    ratings, ids_pair, ids_ui, labels, keep, seed_epoch_key,
                                                                    drop_threshold, unk);
    else
      review_collate_sampled_kernel<false><<<grid, kThreads, 0, s>>>(chunk, first, B, S, L, S_ui, L_ui, pad, tokens, sent_off, n_sent,
                                                                     Role{ptr_u, sid_u}, Role{ptr_i, sid_i}, Role{ptr_ui, sid_ui},
                                                                     ratings, ids_pair, ids_ui, labels, keep, seed_epoch_key,
                                                                     drop_threshold, unk);
    UMPR_LAUNCH_CHECK("review_collate_sampled");
  }
  return 0;
}
