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
