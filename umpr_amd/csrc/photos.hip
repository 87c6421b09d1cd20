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
