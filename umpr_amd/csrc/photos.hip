// Photo resize on the GPU: the loader (umpr_amd/photos.py) ships each photo as the uint8 source pixels its resize taps read,
// plus the tap tables it computed on the host; this kernel finishes umpr_amd/data.py::get_image - OpenCV's 8-bit INTER_LINEAR
// fixed-point resize (data.resize_bilinear_u8) and the division by 255 - and writes the float32 [n][3][dh][dw] photo tensor
// UMPR consumes.  Integer arithmetic throughout and a 256-entry table for k / 255, so the result is bit-identical to the host
// path.  The tables are not recomputed here: hipcc contracts the float coordinate arithmetic into FMAs, numpy does not.
//
// The descriptors are read on the host (the caller passes them in host memory) and validated against the packed buffer's size,
// then travel in the kernel arguments, in chunks of kPhotoChunk photos per launch: no descriptor can make the kernel read outside
// the buffer, and the launch needs no hipMemcpy (capture-safe).  The tap indices themselves live in device memory; the kernel
// clamps them to the photo's compacted source, so a corrupt table gives a wrong picture, never an out-of-bounds read.
#include <algorithm>
#include <vector>

#include "umpr_common.h"
#include "../../include/umpr_hip.h"

namespace {

constexpr int kPhotoChunk = 64;   // 64 x 24 B of kernel arguments per launch, well inside the 4 KB kernarg segment
constexpr int kThreads = 256;

struct PhotoSrc {
  const uint8_t* pix;    // [rows][cols][3]
  const int32_t* taps;   // cx0[dw] cx1[dw] ax0[dw] ax1[dw] ry0[dh] ry1[dh] by0[dh] by1[dh]
  int rows, cols;        // 0 x 0: missing photo
};
struct PhotoChunk {
  PhotoSrc p[kPhotoChunk];
};

// lut[k] = float32(k / 255.0 in float64): what get_image's float64 division followed by batch_loader's float32 cast gives.
struct Lut {
  float v[256];
  constexpr Lut() : v() {
    for (int k = 0; k < 256; ++k) v[k] = (float)((double)k / 255.0);
  }
};
__constant__ Lut kLut = Lut();

// One thread per output pixel; blockIdx.y = photo of the chunk (its descriptor is a wave-uniform kernel-argument load); the
// three channel planes are written with consecutive threads on consecutive pixels of a row.
__global__ __launch_bounds__(kThreads) void photo_resize_u8_kernel(PhotoChunk chunk, int dh, int dw, float* __restrict__ out) {
  __shared__ float lut[256];
  lut[threadIdx.x] = kLut.v[threadIdx.x];
  __syncthreads();
  const int photo = blockIdx.y;
  const int npix = dh * dw;
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= npix) return;
  const PhotoSrc src = chunk.p[photo];
  float* o = out + (size_t)photo * 3 * npix + idx;
  if (src.rows <= 0) {            // missing / unreadable: get_image's except branch
    o[0] = 0.f;
    o[npix] = 0.f;
    o[2 * npix] = 0.f;
    return;
  }
  const int oy = idx / dw, ox = idx - oy * dw;
  const int32_t* t = src.taps;
  const int cx0 = min(max(t[ox], 0), src.cols - 1), cx1 = min(max(t[dw + ox], 0), src.cols - 1);
  const int ax0 = t[2 * dw + ox], ax1 = t[3 * dw + ox];
  const int32_t* ty = t + 4 * dw;
  const int ry0 = min(max(ty[oy], 0), src.rows - 1), ry1 = min(max(ty[dh + oy], 0), src.rows - 1);
  const int by0 = ty[2 * dh + oy], by1 = ty[3 * dh + oy];
  const size_t stride = (size_t)src.cols * 3;
  const uint8_t* r0 = src.pix + ry0 * stride;
  const uint8_t* r1 = src.pix + ry1 * stride;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // horizontal taps, 11-bit weights, >> 4 (OpenCV's HResizeLinear for uchar); then VResizeLinear's rounding
    const int h0 = (r0[cx0 * 3 + c] * ax0 + r0[cx1 * 3 + c] * ax1) >> 4;
    const int h1 = (r1[cx0 * 3 + c] * ax0 + r1[cx1 * 3 + c] * ax1) >> 4;
    const int v = (((by0 * h0) >> 16) + ((by1 * h1) >> 16) + 2) >> 2;
    o[c * npix] = lut[min(max(v, 0), 255)];
  }
}


// ---- device-resident photo store (umpr_amd/photos.py::PhotoStore) --------------------------------------------------------------
// A slot holds the uint8 value behind every output pixel of one resized photo, planar [3][dh][dw] like the float output, padded to
// 16 bytes.  Since the float photo is lut[that byte], a resident photo is reproduced bit for bit without its source pixels.

struct PhotoMiss {
  const uint8_t* pix;
  const int32_t* taps;
  int rows, cols;
  int photo;             // index into this launch's `out`
  int dst_slot;          // slot that receives the uint8 image, or -1
};
struct MissChunk {
  PhotoMiss p[kPhotoChunk];
};
struct PhotoHit {
  int photo, slot;
};
struct HitChunk {
  PhotoHit p[kPhotoChunk];
};

// photo_resize_u8_kernel with one more store per channel: the byte the table lookup reads also goes to the photo's slot.
// kFloat = false (umpr_photo_fetch_augment_u8): the byte only - every record has a source and a dst_slot, `out` is not touched.
template <bool kFloat>
__global__ __launch_bounds__(kThreads) void photo_resize_store_u8_kernel(MissChunk chunk, int dh, int dw, uint8_t* __restrict__ store,
                                                                         size_t slot_bytes, float* __restrict__ out) {
  __shared__ float lut[256];
  if (kFloat) {
    lut[threadIdx.x] = kLut.v[threadIdx.x];
    __syncthreads();
  }
  const int npix = dh * dw;
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= npix) return;
  const PhotoMiss src = chunk.p[blockIdx.y];
  float* o = kFloat ? out + (size_t)src.photo * 3 * npix + idx : nullptr;
  if (kFloat && src.rows <= 0) {  // missing / unreadable: never cached (the host refuses a dst_slot here)
    o[0] = 0.f;
    o[npix] = 0.f;
    o[2 * npix] = 0.f;
    return;
  }
  const int oy = idx / dw, ox = idx - oy * dw;
  const int32_t* t = src.taps;
  const int cx0 = min(max(t[ox], 0), src.cols - 1), cx1 = min(max(t[dw + ox], 0), src.cols - 1);
  const int ax0 = t[2 * dw + ox], ax1 = t[3 * dw + ox];
  const int32_t* ty = t + 4 * dw;
  const int ry0 = min(max(ty[oy], 0), src.rows - 1), ry1 = min(max(ty[dh + oy], 0), src.rows - 1);
  const int by0 = ty[2 * dh + oy], by1 = ty[3 * dh + oy];
  const size_t stride = (size_t)src.cols * 3;
  const uint8_t* r0 = src.pix + ry0 * stride;
  const uint8_t* r1 = src.pix + ry1 * stride;
  uint8_t* keep = src.dst_slot >= 0 ? store + (size_t)src.dst_slot * slot_bytes + idx : nullptr;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h0 = (r0[cx0 * 3 + c] * ax0 + r0[cx1 * 3 + c] * ax1) >> 4;
    const int h1 = (r1[cx0 * 3 + c] * ax0 + r1[cx1 * 3 + c] * ax1) >> 4;
    const int v = min(max((((by0 * h0) >> 16) + ((by1 * h1) >> 16) + 2) >> 2, 0), 255);
    if (kFloat) o[c * npix] = lut[v];
    if (keep) keep[c * npix] = (uint8_t)v;
  }
}

typedef float float4_dw __attribute__((ext_vector_type(4), aligned(4)));   // a photo of an odd pixel count starts 4-byte aligned only

constexpr int kHitBytes = kThreads * 16;   // slot bytes per block

// Resident photos: out[photo][j] = lut[slot[j]], j < n = 3*dh*dw, a contiguous uint8 -> float32 conversion.  A block converts
// kHitBytes bytes of one slot: each thread loads 16 of them (one dwordx4 per lane, 1 KiB per wave), the block turns them over
// through LDS so that thread t holds dword j*256 + t, and stores its four floats as one float4: both the load and the stores of a
// wave are contiguous.  The last n % 16 bytes go one per thread.  kAligned: n % 4 == 0, so every photo of `out` is 16-byte aligned.
template <bool kAligned>
__global__ __launch_bounds__(kThreads) void photo_fetch_u8_kernel(HitChunk chunk, int n, const uint8_t* __restrict__ store,
                                                                  size_t slot_bytes, float* __restrict__ out) {
  __shared__ float lut[256];
  __shared__ uint4 stage[kThreads];
  const int tid = threadIdx.x;
  lut[tid] = kLut.v[tid];
  const PhotoHit hit = chunk.p[blockIdx.y];
  const uint8_t* s = store + (size_t)hit.slot * slot_bytes;
  float* o = out + (size_t)hit.photo * n;
  const int nvec = n & ~15;
  const int base = blockIdx.x * kHitBytes;
  if (base + tid * 16 < nvec) stage[tid] = *reinterpret_cast<const uint4*>(s + base + tid * 16);
  __syncthreads();
  const uint32_t* words = reinterpret_cast<const uint32_t*>(stage);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = j * kThreads + tid;
    const int e = base + d * 4;
    if (e < nvec) {                 // nvec is a multiple of 16: the 16-byte group of dword d was loaded
      const uint32_t w = words[d];
      const float f0 = lut[w & 255], f1 = lut[(w >> 8) & 255], f2 = lut[(w >> 16) & 255], f3 = lut[w >> 24];
      if (kAligned) {
        *reinterpret_cast<float4*>(o + e) = make_float4(f0, f1, f2, f3);
      } else {
        float4_dw f = {f0, f1, f2, f3};
        *reinterpret_cast<float4_dw*>(o + e) = f;
      }
    }
  }
  if (blockIdx.x == gridDim.x - 1 && tid < n - nvec) o[nvec + tid] = lut[s[nvec + tid]];
}

// ---- augmented fetch (umpr_amd/photos.py::PhotoAugment) -----------------------------------------------------------------------------
// The float photo of a crop window of a slot, resized back to dh x dw by the same integer INTER_LINEAR and mirrored or not:
// data.resize_bilinear_u8 on U[y0:y0+ch, x0:x0+cw], U the slot's image.  The taps of every source extent 1..dw / 1..dh were built
// once on the host with the numpy expressions the host resize uses (header of this file): xtaps [dw][4][dw], row cw-1 = x0 x1 a0 a1
// of _column_taps(dw, cw); ytaps [dh][4][dh] likewise from _row_taps.  The kernel clamps the indices into the window, which the
// host has checked to lie inside the image: a corrupt table gives a wrong picture, never a read outside the slot.

struct PhotoAug {
  int slot;              // of `store`, or of `scratch` with kAugScratch; unused with kAugMissing
  int x0, y0, cw, ch;    // the window
  int mode;              // kAugFlip | kAugScratch | kAugMissing
};
struct AugChunk {
  PhotoAug p[kPhotoChunk];
};
constexpr int kAugFlip = 1, kAugScratch = 2, kAugMissing = 4;
static_assert(sizeof(AugChunk) == kPhotoChunk * 24, "64 x 24 B of kernel arguments per launch, well inside the 4 KB kernarg segment");

constexpr int kAugRows = 8, kAugCols = kThreads;   // the output tile of a block: one thread per column in the horizontal pass
constexpr int kAugMaxSide = 4096;
// A window is never larger than the image, so the resize only magnifies: kAugCols consecutive output columns tap at most
// kAugCols + 1 consecutive source columns, kAugRows output rows at most kAugRows + 1 source rows.  (In exact arithmetic; the
// coordinate is rounded to float32, which can cost one more only beyond 7000 pixels a side, and the host refuses sides above
// kAugMaxSide.)  A table that asks for more is clamped to what is staged: a wrong picture, no read outside LDS or the slot.
constexpr int kAugSrcRows = kAugRows + 1, kAugSrcCols = kAugCols + 1, kAugSrcPitch = kAugCols + 4;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// A block makes a kAugRows x kAugCols tile of one photo (blockIdx.y: its record is a wave-uniform kernel-argument load), all three
// planes, in three steps through LDS: (1) the source rows and columns the tile taps are staged as bytes, consecutive threads on
// consecutive bytes of a row, while each thread also loads the taps of its column; (2) the horizontal pass, one thread per output
// column, leaves HResizeLinear's 16-bit sums (at most 255 * 2048 >> 4) of every staged row; (3) the vertical pass and the table
// lookup, kVec ? four : one output pixel per thread, stored as one float4 (kVec: dw % 4 == 0, so every row of every plane of `out`
// is 16-byte aligned) or float.  A flip reverses the column whose taps a thread loads, nothing else.  22 KB of LDS: seven blocks
// on a CU, so the 28 x 64 blocks of 64 photos at 224 x 224 are all resident at once on 256 CUs.  How this form and the
// one-thread-per-pixel form of photo_resize_u8_kernel compare with the plain fetch: profiles/r17_a_photo_augment.txt.
template <bool kVec>
__global__ __launch_bounds__(kThreads) void photo_augment_u8_kernel(AugChunk chunk, int dh, int dw, const uint8_t* __restrict__ store,
                                                                    const uint8_t* __restrict__ scratch, size_t slot_bytes,
                                                                    const int32_t* __restrict__ xtaps,
                                                                    const int32_t* __restrict__ ytaps, float* __restrict__ out) {
  constexpr int W = kVec ? 4 : 1;
  __shared__ float lut[256];
  __shared__ uint8_t src[3][kAugSrcRows][kAugSrcPitch];
  __shared__ uint16_t hsum[3][kAugSrcRows][kAugCols];
  __shared__ int ytap[kAugRows][4];        // per output row of the tile: its two staged rows and their weights
  const int tid = threadIdx.x;
  lut[tid] = kLut.v[tid];
  const PhotoAug a = chunk.p[blockIdx.y];
  const int npix = dh * dw;
  const int tiles_x = (dw + kAugCols - 1) / kAugCols;
  const int tile_y = blockIdx.x / tiles_x;
  const int ox0 = (blockIdx.x - tile_y * tiles_x) * kAugCols, oy0 = tile_y * kAugRows;
  const int nx = min(kAugCols, dw - ox0), ny = min(kAugRows, dh - oy0);
  const int groups = (nx + W - 1) / W;     // kVec: ox0 and dw are multiples of 4, so nx is one too
  float* o = out + (size_t)blockIdx.y * 3 * npix + (size_t)oy0 * dw + ox0;
  if (a.mode & kAugMissing) {              // the whole block: nobody reaches a barrier
    for (int k = tid; k < ny * groups; k += kThreads) {
      const int yl = k / groups, g = k - yl * groups;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float* q = o + (size_t)c * npix + yl * dw + g * W;
        if (kVec)
          *reinterpret_cast<float4*>(q) = make_float4(0.f, 0.f, 0.f, 0.f);
        else
          *q = 0.f;
      }
    }
    return;
  }
  const bool flip = a.mode & kAugFlip;
  const int32_t* t = xtaps + (size_t)(a.cw - 1) * 4 * dw;
  const int32_t* ty = ytaps + (size_t)(a.ch - 1) * 4 * dh;
  // the tile's output columns read the taps of the columns ta .. ta + nx - 1 (ascending also when flipped)
  const int ta = flip ? dw - ox0 - nx : ox0;
  const int clo = clampi(t[ta], 0, a.cw - 1), rlo = clampi(ty[oy0], 0, a.ch - 1);
  const int ncols = clampi(clampi(t[dw + ta + nx - 1], 0, a.cw - 1) - clo + 1, 1, kAugSrcCols);
  const int nrows = clampi(clampi(ty[dh + oy0 + ny - 1], 0, a.ch - 1) - rlo + 1, 1, kAugSrcRows);
  // this thread's column of the tile (nx <= kAugCols = kThreads), its taps relative to what is staged
  const int tx = flip ? dw - 1 - (ox0 + tid) : ox0 + tid;
  int c0 = 0, c1 = 0, a0 = 0, a1 = 0;
  if (tid < nx) {
    c0 = clampi(clampi(t[tx], 0, a.cw - 1) - clo, 0, ncols - 1);
    c1 = clampi(clampi(t[dw + tx], 0, a.cw - 1) - clo, 0, ncols - 1);
    a0 = t[2 * dw + tx];
    a1 = t[3 * dw + tx];
  }
  if (tid < ny) {
    const int oy = oy0 + tid;
    ytap[tid][0] = clampi(clampi(ty[oy], 0, a.ch - 1) - rlo, 0, nrows - 1);
    ytap[tid][1] = clampi(clampi(ty[dh + oy], 0, a.ch - 1) - rlo, 0, nrows - 1);
    ytap[tid][2] = ty[2 * dh + oy];
    ytap[tid][3] = ty[3 * dh + oy];
  }
  // (1) rows y0 + rlo .. + nrows - 1, columns x0 + clo .. + ncols - 1: inside the window, which the host checked to be inside the slot
  const uint8_t* s = ((a.mode & kAugScratch) ? scratch : store) + (size_t)a.slot * slot_bytes + (size_t)(a.y0 + rlo) * dw + a.x0 + clo;
#pragma unroll
  for (int r = 0; r < kAugSrcRows; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (r < nrows && tid < ncols) src[c][r][tid] = s[(size_t)c * npix + r * dw + tid];
  }
  if (ncols > kThreads && tid < 3 * kAugSrcRows) {        // the one column more than there are threads
    const int c = tid / kAugSrcRows, r = tid - c * kAugSrcRows;
    if (r < nrows) src[c][r][kThreads] = s[(size_t)c * npix + r * dw + kThreads];
  }
  __syncthreads();
  // (2) horizontal taps, 11-bit weights, >> 4 (OpenCV's HResizeLinear for uchar)
  if (tid < nx) {
#pragma unroll
    for (int r = 0; r < kAugSrcRows; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (r < nrows) hsum[c][r][tid] = (uint16_t)((src[c][r][c0] * a0 + src[c][r][c1] * a1) >> 4);
    }
  }
  __syncthreads();
  // (3) VResizeLinear's rounding, then k / 255 from the table
  for (int k = tid; k < ny * groups; k += kThreads) {
    const int yl = k / groups, g = k - yl * groups;
    const int r0 = ytap[yl][0], r1 = ytap[yl][1], b0 = ytap[yl][2], b1 = ytap[yl][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float f[W];
#pragma unroll
      for (int p = 0; p < W; ++p) {
        const int v = (((b0 * (int)hsum[c][r0][g * W + p]) >> 16) + ((b1 * (int)hsum[c][r1][g * W + p]) >> 16) + 2) >> 2;
        f[p] = lut[clampi(v, 0, 255)];
      }
      float* q = o + (size_t)c * npix + yl * dw + g * W;
      if (kVec)
        *reinterpret_cast<float4*>(q) = make_float4(f[0], f[W > 1 ? 1 : 0], f[W > 2 ? 2 : 0], f[W > 3 ? 3 : 0]);
      else
        *q = f[0];
    }
  }
}

// ---- device-resident VGG features (umpr_amd/photos.py::FeatureStore) ---------------------------------------------------------------
// With a frozen VGG the F = 1000 floats behind a photo are a constant of the run: a slot holds them, and a resident photo costs one
// row copy instead of a resize and a VGG forward.

struct FeatRow {
  int src_slot;          // >= 0: the row is read from this slot of the store
  int fresh_row;         // else: from this row of `fresh`
  int dst_slot;          // >= 0: the row is also written to this slot
};
struct FeatChunk {
  FeatRow r[kPhotoChunk];
};

// out[row] = store[src_slot] or fresh[fresh_row], and the same 16-byte groups to store[dst_slot]: one uint4 per thread, blockIdx.y
// = row of the chunk (its record is a wave-uniform kernel-argument load).  The host has checked that no dst_slot of the call is
// read or written twice, so the launch has no ordering of its own to keep.
__global__ __launch_bounds__(kThreads) void feature_fetch_f32_kernel(FeatChunk chunk, int nvec, const uint4* __restrict__ fresh,
                                                                     uint4* store, uint4* __restrict__ out) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= nvec) return;
  const FeatRow r = chunk.r[blockIdx.y];
  const uint4* s = r.src_slot >= 0 ? store + (size_t)r.src_slot * nvec : fresh + (size_t)r.fresh_row * nvec;
  const uint4 v = s[j];
  out[(size_t)blockIdx.y * nvec + j] = v;
  if (r.dst_slot >= 0) store[(size_t)r.dst_slot * nvec + j] = v;
}

}  // namespace

extern "C" int umpr_photo_resize_u8(const uint8_t* packed, size_t packed_bytes, const umpr_photo_desc* desc, int n_photos,
                                    int dst_h, int dst_w, float* out, void* stream) {
  UMPR_REQUIRE(n_photos >= 0, "photo_resize_u8: n_photos = %d", n_photos);
  if (n_photos == 0) return 0;
  UMPR_REQUIRE(desc != nullptr && out != nullptr, "photo_resize_u8: null argument");
  UMPR_REQUIRE(dst_h > 0 && dst_w > 0 && (long)dst_h * dst_w <= (1L << 24), "photo_resize_u8: bad output size %d x %d",
               dst_h, dst_w);
  const long tap_bytes = 16L * (dst_w + dst_h);
  for (int i = 0; i < n_photos; ++i) {
    const umpr_photo_desc& d = desc[i];
    if (d.rows == 0 && d.cols == 0) continue;
    UMPR_REQUIRE(packed != nullptr, "photo_resize_u8: null packed buffer");
    UMPR_REQUIRE(d.rows > 0 && d.cols > 0 && d.rows <= (1 << 20) && d.cols <= (1 << 20),
                 "photo_resize_u8: photo %d has a %d x %d source", i, d.rows, d.cols);
    UMPR_REQUIRE(d.taps >= 0 && d.taps % 4 == 0 && (uint64_t)d.taps + tap_bytes <= packed_bytes,
                 "photo_resize_u8: photo %d: tap tables at byte %lld (+%ld) outside the %zu-byte buffer or misaligned", i,
                 (long long)d.taps, tap_bytes, packed_bytes);
    UMPR_REQUIRE(d.pixels >= 0 && (uint64_t)d.pixels + 3ull * (uint64_t)d.rows * (uint64_t)d.cols <= packed_bytes,
                 "photo_resize_u8: photo %d: %d x %d pixels at byte %lld outside the %zu-byte buffer", i, d.rows, d.cols,
                 (long long)d.pixels, packed_bytes);
  }
  UMPR_REQUIRE(((uintptr_t)packed & 3) == 0, "photo_resize_u8: packed buffer not 4-byte aligned");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int npix = dst_h * dst_w;
  for (int first = 0; first < n_photos; first += kPhotoChunk) {
    const int n = min(kPhotoChunk, n_photos - first);
    PhotoChunk chunk = {};
    for (int i = 0; i < n; ++i) {
      const umpr_photo_desc& d = desc[first + i];
      const bool have = d.rows > 0;
      chunk.p[i] = {have ? packed + d.pixels : nullptr, have ? reinterpret_cast<const int32_t*>(packed + d.taps) : nullptr,
                    have ? d.rows : 0, have ? d.cols : 0};
    }
    photo_resize_u8_kernel<<<dim3(cdiv(npix, kThreads), n), kThreads, 0, s>>>(chunk, dst_h, dst_w,
                                                                                out + (size_t)first * 3 * npix);
    UMPR_LAUNCH_CHECK("photo_resize_u8");
  }
  return 0;
}

extern "C" size_t umpr_photo_store_slot_bytes(int dst_h, int dst_w) {
  if (dst_h <= 0 || dst_w <= 0 || (long)dst_h * dst_w > (1L << 24)) return 0;
  return ((size_t)3 * dst_h * dst_w + 15) & ~(size_t)15;
}

// What umpr_photo_fetch_u8 and umpr_photo_fetch_augment_u8 refuse alike, before any launch: `fn` names the caller in the message.
static int check_photo_fetch(const char* fn, const uint8_t* packed, size_t packed_bytes, const umpr_photo_desc* desc,
                             const int32_t* src_slot, const int32_t* dst_slot, int n_photos, int dst_h, int dst_w,
                             const uint8_t* store, long n_slots, const float* out) {
  UMPR_REQUIRE(desc != nullptr && src_slot != nullptr && dst_slot != nullptr && out != nullptr, "%s: null argument", fn);
  UMPR_REQUIRE(dst_h > 0 && dst_w > 0 && (long)dst_h * dst_w <= (1L << 24), "%s: bad output size %d x %d", fn, dst_h,
               dst_w);
  UMPR_REQUIRE(n_slots >= 0 && n_slots <= 0x7fffffffL, "%s: n_slots = %ld", fn, n_slots);
  const long tap_bytes = 16L * (dst_w + dst_h);
  std::vector<int32_t> written;
  for (int i = 0; i < n_photos; ++i) {
    const umpr_photo_desc& d = desc[i];
    const bool empty = d.rows == 0 && d.cols == 0;
    if (src_slot[i] >= 0 || dst_slot[i] >= 0) {
      UMPR_REQUIRE(store != nullptr, "%s: photo %d uses a slot but the store is null", fn, i);
      const int32_t slot = src_slot[i] >= 0 ? src_slot[i] : dst_slot[i];
      UMPR_REQUIRE(slot < n_slots, "%s: photo %d: slot %d outside the %ld-slot store", fn, i, slot, n_slots);
    }
    if (src_slot[i] >= 0) {
      UMPR_REQUIRE(dst_slot[i] < 0, "%s: photo %d has both a src_slot and a dst_slot", fn, i);
      UMPR_REQUIRE(empty, "%s: photo %d is read from slot %d but carries a %d x %d source", fn, i, src_slot[i], d.rows,
                   d.cols);
      continue;
    }
    if (dst_slot[i] >= 0) {
      UMPR_REQUIRE(!empty, "%s: photo %d has no source to fill slot %d with", fn, i, dst_slot[i]);
      written.push_back(dst_slot[i]);
    }
    if (empty) continue;
    UMPR_REQUIRE(packed != nullptr, "%s: null packed buffer", fn);
    UMPR_REQUIRE(d.rows > 0 && d.cols > 0 && d.rows <= (1 << 20) && d.cols <= (1 << 20),
                 "%s: photo %d has a %d x %d source", fn, i, d.rows, d.cols);
    UMPR_REQUIRE(d.taps >= 0 && d.taps % 4 == 0 && (uint64_t)d.taps + tap_bytes <= packed_bytes,
                 "%s: photo %d: tap tables at byte %lld (+%ld) outside the %zu-byte buffer or misaligned", fn, i,
                 (long long)d.taps, tap_bytes, packed_bytes);
    UMPR_REQUIRE(d.pixels >= 0 && (uint64_t)d.pixels + 3ull * (uint64_t)d.rows * (uint64_t)d.cols <= packed_bytes,
                 "%s: photo %d: %d x %d pixels at byte %lld outside the %zu-byte buffer", fn, i, d.rows, d.cols,
                 (long long)d.pixels, packed_bytes);
  }
  std::sort(written.begin(), written.end());
  for (size_t k = 1; k < written.size(); ++k)
    UMPR_REQUIRE(written[k] != written[k - 1], "%s: slot %d is the dst_slot of two photos", fn, written[k]);
  for (int i = 0; i < n_photos; ++i)
    UMPR_REQUIRE(src_slot[i] < 0 || !std::binary_search(written.begin(), written.end(), src_slot[i]),
                 "%s: photo %d reads slot %d, which this call writes", fn, i, src_slot[i]);
  UMPR_REQUIRE(((uintptr_t)packed & 3) == 0, "%s: packed buffer not 4-byte aligned", fn);
  UMPR_REQUIRE(((uintptr_t)store & 15) == 0 && ((uintptr_t)out & 15) == 0, "%s: store or out not 16-byte aligned", fn);
  return 0;
}

extern "C" int umpr_photo_fetch_u8(const uint8_t* packed, size_t packed_bytes, const umpr_photo_desc* desc,
                                   const int32_t* src_slot, const int32_t* dst_slot, int n_photos, int dst_h, int dst_w,
                                   uint8_t* store, long n_slots, float* out, void* stream) {
  UMPR_REQUIRE(n_photos >= 0, "photo_fetch_u8: n_photos = %d", n_photos);
  if (n_photos == 0) return 0;
  if (check_photo_fetch("photo_fetch_u8", packed, packed_bytes, desc, src_slot, dst_slot, n_photos, dst_h, dst_w, store, n_slots,
                        out))
    return -1;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int npix = dst_h * dst_w, n = 3 * npix;
  const size_t slot_bytes = umpr_photo_store_slot_bytes(dst_h, dst_w);
  for (int first = 0; first < n_photos; first += kPhotoChunk) {
    const int cnt = min(kPhotoChunk, n_photos - first);
    MissChunk miss = {};
    HitChunk hit = {};
    int n_miss = 0, n_hit = 0;
    for (int i = 0; i < cnt; ++i) {
      const umpr_photo_desc& d = desc[first + i];
      if (src_slot[first + i] >= 0) {
        hit.p[n_hit++] = {i, src_slot[first + i]};
        continue;
      }
      const bool have = d.rows > 0;
      miss.p[n_miss++] = {have ? packed + d.pixels : nullptr, have ? reinterpret_cast<const int32_t*>(packed + d.taps) : nullptr,
                          have ? d.rows : 0, have ? d.cols : 0, i, have ? dst_slot[first + i] : -1};
    }
    float* o = out + (size_t)first * n;
    if (n_miss) {
      photo_resize_store_u8_kernel<true><<<dim3(cdiv(npix, kThreads), n_miss), kThreads, 0, s>>>(miss, dst_h, dst_w, store, slot_bytes, o);
      UMPR_LAUNCH_CHECK("photo_fetch_u8 (resize)");
    }
    if (n_hit) {
      const dim3 grid(cdiv(n, kHitBytes), n_hit);
      if (n % 4 == 0)
        photo_fetch_u8_kernel<true><<<grid, kThreads, 0, s>>>(hit, n, store, slot_bytes, o);
      else
        photo_fetch_u8_kernel<false><<<grid, kThreads, 0, s>>>(hit, n, store, slot_bytes, o);
      UMPR_LAUNCH_CHECK("photo_fetch_u8 (fetch)");
    }
  }
  return 0;
}

extern "C" int umpr_photo_fetch_augment_u8(const uint8_t* packed, size_t packed_bytes, const umpr_photo_desc* desc,
                                           const int32_t* src_slot, const int32_t* dst_slot, const int32_t* crop, int n_photos,
                                           int dst_h, int dst_w, uint8_t* store, long n_slots, uint8_t* scratch, long n_scratch,
                                           const int32_t* xtaps, const int32_t* ytaps, float* out, void* stream) {
  const char* fn = "photo_fetch_augment_u8";
  UMPR_REQUIRE(n_photos >= 0, "%s: n_photos = %d", fn, n_photos);
  if (n_photos == 0) return 0;
  if (check_photo_fetch(fn, packed, packed_bytes, desc, src_slot, dst_slot, n_photos, dst_h, dst_w, store, n_slots, out)) return -1;
  UMPR_REQUIRE(dst_h <= kAugMaxSide && dst_w <= kAugMaxSide, "%s: output size %d x %d has a side above %d", fn, dst_h, dst_w,
               kAugMaxSide);
  UMPR_REQUIRE(crop != nullptr, "%s: null crop records", fn);
  UMPR_REQUIRE(xtaps != nullptr && ytaps != nullptr, "%s: null tap table", fn);
  UMPR_REQUIRE(((uintptr_t)xtaps & 3) == 0 && ((uintptr_t)ytaps & 3) == 0, "%s: tap tables not 4-byte aligned", fn);
  UMPR_REQUIRE(n_scratch >= 0 && n_scratch <= 0x7fffffffL, "%s: n_scratch = %ld", fn, n_scratch);
  long need = 0;   // decoded photos without a dst_slot: each takes the next scratch slot
  for (int i = 0; i < n_photos; ++i) {
    const int32_t* w = crop + 5 * (size_t)i;
    UMPR_REQUIRE(w[2] >= 1 && w[3] >= 1, "%s: photo %d: empty window %d x %d", fn, i, w[2], w[3]);
    UMPR_REQUIRE(w[0] >= 0 && w[1] >= 0 && w[2] <= dst_w - w[0] && w[3] <= dst_h - w[1],
                 "%s: photo %d: window %d x %d at (%d, %d) outside the %d x %d image", fn, i, w[2], w[3], w[0], w[1], dst_w, dst_h);
    UMPR_REQUIRE(w[4] == 0 || w[4] == 1, "%s: photo %d: flip = %d, not 0 or 1", fn, i, w[4]);
    if (src_slot[i] < 0 && dst_slot[i] < 0 && desc[i].rows > 0) {
      UMPR_REQUIRE(need < n_scratch, "%s: photo %d: decoded without a dst_slot, and all %ld scratch slots are taken", fn, i,
                   n_scratch);
      ++need;
    }
  }
  UMPR_REQUIRE(need == 0 || scratch != nullptr, "%s: %ld photos need a scratch slot but scratch is null", fn, need);
  UMPR_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch not 16-byte aligned", fn);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int npix = dst_h * dst_w;
  const size_t slot_bytes = umpr_photo_store_slot_bytes(dst_h, dst_w);
  int next_scratch = 0;
  for (int first = 0; first < n_photos; first += kPhotoChunk) {
    const int cnt = min(kPhotoChunk, n_photos - first);
    MissChunk to_store = {}, to_scratch = {};   // the decoded photos of the chunk, by where their plain uint8 image goes
    AugChunk aug = {};
    int n_store = 0, n_scr = 0;
    for (int i = 0; i < cnt; ++i) {
      const umpr_photo_desc& d = desc[first + i];
      const int32_t* w = crop + 5 * (size_t)(first + i);
      int slot = src_slot[first + i], mode = w[4] ? kAugFlip : 0;
      if (slot < 0 && d.rows <= 0) {
        mode = kAugMissing;
        slot = 0;
      } else if (slot < 0) {
        const bool keep = dst_slot[first + i] >= 0;
        slot = keep ? dst_slot[first + i] : next_scratch++;
        if (!keep) mode |= kAugScratch;
        (keep ? to_store.p[n_store++] : to_scratch.p[n_scr++]) = {packed + d.pixels, reinterpret_cast<const int32_t*>(packed + d.taps),
                                                                  d.rows, d.cols, i, slot};
      }
      aug.p[i] = {slot, w[0], w[1], w[2], w[3], mode};
    }
    // a store slot always receives the plain image; the one augment launch below reads it back on the same stream
    if (n_store) {
      photo_resize_store_u8_kernel<false><<<dim3(cdiv(npix, kThreads), n_store), kThreads, 0, s>>>(to_store, dst_h, dst_w, store,
                                                                                                    slot_bytes, nullptr);
      UMPR_LAUNCH_CHECK("photo_fetch_augment_u8 (resize to store)");
    }
    if (n_scr) {
      photo_resize_store_u8_kernel<false><<<dim3(cdiv(npix, kThreads), n_scr), kThreads, 0, s>>>(to_scratch, dst_h, dst_w, scratch,
                                                                                                  slot_bytes, nullptr);
      UMPR_LAUNCH_CHECK("photo_fetch_augment_u8 (resize to scratch)");
    }
    const dim3 grid(cdiv(dst_w, kAugCols) * cdiv(dst_h, kAugRows), cnt);
    float* o = out + (size_t)first * 3 * npix;
    if (dst_w % 4 == 0)
      photo_augment_u8_kernel<true><<<grid, kThreads, 0, s>>>(aug, dst_h, dst_w, store, scratch, slot_bytes, xtaps, ytaps, o);
    else
      photo_augment_u8_kernel<false><<<grid, kThreads, 0, s>>>(aug, dst_h, dst_w, store, scratch, slot_bytes, xtaps, ytaps, o);
    UMPR_LAUNCH_CHECK("photo_fetch_augment_u8 (augment)");
  }
  return 0;
}

extern "C" int umpr_feature_fetch_f32(const float* fresh, int n_fresh, const int32_t* fresh_row, const int32_t* src_slot,
                                      const int32_t* dst_slot, int n, int F, float* store, long n_slots, float* out, void* stream) {
  UMPR_REQUIRE(n >= 0 && n_fresh >= 0, "feature_fetch_f32: n = %d, n_fresh = %d", n, n_fresh);
  if (n == 0) return 0;
  UMPR_REQUIRE(fresh_row != nullptr && src_slot != nullptr && dst_slot != nullptr && out != nullptr,
               "feature_fetch_f32: null argument");
  UMPR_REQUIRE(F > 0 && F % 4 == 0 && F <= (1 << 24), "feature_fetch_f32: F = %d is not a positive multiple of 4", F);
  UMPR_REQUIRE(n_slots >= 0 && n_slots <= 0x7fffffffL, "feature_fetch_f32: n_slots = %ld", n_slots);
  UMPR_REQUIRE(n_fresh == 0 || fresh != nullptr, "feature_fetch_f32: %d fresh rows but a null `fresh`", n_fresh);
  UMPR_REQUIRE(((uintptr_t)fresh & 15) == 0 && ((uintptr_t)store & 15) == 0 && ((uintptr_t)out & 15) == 0,
               "feature_fetch_f32: fresh, store or out not 16-byte aligned");
  std::vector<int32_t> written;
  for (int i = 0; i < n; ++i) {
    const bool hit = src_slot[i] >= 0, computed = fresh_row[i] >= 0;
    UMPR_REQUIRE(hit != computed, "feature_fetch_f32: photo %d has %s a src_slot and a fresh_row", i, hit ? "both" : "neither");
    if (hit || dst_slot[i] >= 0) UMPR_REQUIRE(store != nullptr, "feature_fetch_f32: photo %d uses a slot but the store is null", i);
    if (hit) UMPR_REQUIRE(src_slot[i] < n_slots, "feature_fetch_f32: photo %d: src_slot %d outside the %ld-slot store", i,
                          src_slot[i], n_slots);
    if (computed) UMPR_REQUIRE(fresh_row[i] < n_fresh, "feature_fetch_f32: photo %d: fresh_row %d outside the %d fresh rows", i,
                               fresh_row[i], n_fresh);
    if (dst_slot[i] >= 0) {
      UMPR_REQUIRE(dst_slot[i] < n_slots, "feature_fetch_f32: photo %d: dst_slot %d outside the %ld-slot store", i, dst_slot[i],
                   n_slots);
      written.push_back(dst_slot[i]);
    }
  }
  std::sort(written.begin(), written.end());
  for (size_t k = 1; k < written.size(); ++k)
    UMPR_REQUIRE(written[k] != written[k - 1], "feature_fetch_f32: slot %d is the dst_slot of two photos", written[k]);
  for (int i = 0; i < n; ++i)
    UMPR_REQUIRE(src_slot[i] < 0 || !std::binary_search(written.begin(), written.end(), src_slot[i]),
                 "feature_fetch_f32: photo %d reads slot %d, which this call writes", i, src_slot[i]);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int nvec = F / 4;
  for (int first = 0; first < n; first += kPhotoChunk) {
    const int cnt = min(kPhotoChunk, n - first);
    FeatChunk chunk = {};
    for (int i = 0; i < cnt; ++i)
      chunk.r[i] = {src_slot[first + i] >= 0 ? src_slot[first + i] : -1, src_slot[first + i] >= 0 ? -1 : fresh_row[first + i],
                    dst_slot[first + i] >= 0 ? dst_slot[first + i] : -1};
    feature_fetch_f32_kernel<<<dim3(cdiv(nvec, kThreads), cnt), kThreads, 0, s>>>(
        chunk, nvec, reinterpret_cast<const uint4*>(fresh), reinterpret_cast<uint4*>(store),
        reinterpret_cast<uint4*>(out + (size_t)first * F));
    UMPR_LAUNCH_CHECK("feature_fetch_f32");
  }
  return 0;
}
