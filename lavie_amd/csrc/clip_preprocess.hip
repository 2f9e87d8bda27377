// CLIPImageProcessor on the device: Pillow's 8-bit bicubic resampling of the columns and rows the centre crop keeps,
// then the fp32 normalisation, from uint8 [B, H, W, 3] to [B, 3, crop, crop].
//   clip_resample_h_kernel   source rows [row0, row0 + rows) x kept columns -> mid uint8 [B, rows, crop, 3] (Pillow's horizontal pass)
//   clip_resample_v_kernel   mid -> out[b, c, y, x] = lut[c][pixel]          (Pillow's vertical pass, then the 768-entry table)
// Both passes are Pillow's integer arithmetic: a signed 32-bit accumulator that starts at 2^21, the taps' coefficients as int32 scaled by
// 2^22 (made on the host in double, clip_engine.cpp), an arithmetic shift by 22 and a clip to 0 .. 255.  There is no floating point
// on the device: the value stored is an entry of the table the host made with true fp32 divisions, so an element has the stock
// processor's bits; the fp16 output is ONE rounding of that entry.  An output element reads its own taps only: nothing depends on B or
// on the image's position.  No source byte outside [0, H) x [0, 3 W) of an image is addressed: a tap row ends at xmin + count <= W.
// The tables cover the kept outputs only, so rows and columns the crop discards are never read.
#include "common.h"
#include "ops.h"

namespace lavie {

namespace {

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> 22;               // arithmetic shift of the signed accumulator, as Pillow's clip8
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// grid (ceil(3 crop / 256), rows, B): thread = one byte (column x, channel c) of one source row
__global__ __launch_bounds__(256) void clip_resample_h_kernel(const uint8_t* __restrict__ in, size_t row_pitch, size_t image_pitch,
                                                              uint8_t* __restrict__ mid, int row0, int rows, int crop,
                                                              const int* __restrict__ xmin, const int* __restrict__ cnt,
                                                              const int* __restrict__ coeff, int ksize) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= 3 * crop) return;
    const int x = j / 3, c = j - 3 * x;
    const int r = blockIdx.y, b = blockIdx.z;
    const uint8_t* src = in + (size_t)b * image_pitch + (size_t)(row0 + r) * row_pitch + (size_t)xmin[x] * 3 + c;
    const int* k = coeff + (size_t)x * ksize;
    const int n = cnt[x];
    int acc = 1 << 21;
    for (int t = 0; t < n; ++t) acc += (int)src[3 * t] * k[t];
    mid[((size_t)b * rows + r) * (3 * (size_t)crop) + j] = (uint8_t)clip8(acc);
}

// grid (ceil(crop / 256), crop, B): thread = the three channels of one output pixel; ymin is relative to the first row of mid
template <typename T>
__global__ __launch_bounds__(256) void clip_resample_v_kernel(const uint8_t* __restrict__ mid, T* __restrict__ out, int rows, int crop,
                                                              const int* __restrict__ ymin, const int* __restrict__ cnt,
                                                              const int* __restrict__ coeff, int ksize, const float* __restrict__ lut) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= crop) return;
    const int y = blockIdx.y, b = blockIdx.z;
    const size_t pitch = 3 * (size_t)crop;
    const uint8_t* src = mid + ((size_t)b * rows + ymin[y]) * pitch + 3 * (size_t)x;
    const int* k = coeff + (size_t)y * ksize;
    const int n = cnt[y];
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int t = 0; t < n; ++t) {
        const int kk = k[t];
        const uint8_t* p = src + (size_t)t * pitch;
        a0 += (int)p[0] * kk;
        a1 += (int)p[1] * kk;
        a2 += (int)p[2] * kk;
    }
    const size_t plane = (size_t)crop * crop;
    T* o = out + (size_t)b * 3 * plane + (size_t)y * crop + x;
    o[0] = (T)lut[clip8(a0)];
    o[plane] = (T)lut[256 + clip8(a1)];
    o[2 * plane] = (T)lut[512 + clip8(a2)];
}

}  // namespace

int launch_clip_resample_h(const uint8_t* in, long long row_pitch, long long image_pitch, uint8_t* mid, int B, int row0, int rows, int crop,
                           const int* xmin, const int* cnt, const int* coeff, int ksize, hipStream_t stream) {
    LAVIE_CHECK(in && mid && xmin && cnt && coeff, "clip_preprocess: null tensor");
    LAVIE_CHECK(B >= 1 && B <= 65535 && rows >= 1 && rows <= 65535 && crop >= 1 && ksize >= 1, "clip_preprocess: B=%d rows=%d crop=%d", B, rows,
                crop);
    const dim3 grid((unsigned)cdiv(3 * crop, 256), (unsigned)rows, (unsigned)B);
    hipLaunchKernelGGL(clip_resample_h_kernel, grid, dim3(256), 0, stream, in, (size_t)row_pitch, (size_t)image_pitch, mid, row0, rows, crop,
                       xmin, cnt, coeff, ksize);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_clip_resample_v(const uint8_t* mid, void* out, bool out_f32, int B, int rows, int crop, const int* ymin, const int* cnt,
                           const int* coeff, int ksize, const float* lut, hipStream_t stream) {
    LAVIE_CHECK(mid && out && ymin && cnt && coeff && lut, "clip_preprocess: null tensor");
    LAVIE_CHECK(B >= 1 && B <= 65535 && rows >= 1 && crop >= 1 && crop <= 65535 && ksize >= 1, "clip_preprocess: B=%d rows=%d crop=%d", B, rows,
                crop);
    const dim3 grid((unsigned)cdiv(crop, 256), (unsigned)crop, (unsigned)B);
    if (out_f32)
        hipLaunchKernelGGL(clip_resample_v_kernel<float>, grid, dim3(256), 0, stream, mid, (float*)out, rows, crop, ymin, cnt, coeff, ksize, lut);
    else
        hipLaunchKernelGGL(clip_resample_v_kernel<half_t>, grid, dim3(256), 0, stream, mid, (half_t*)out, rows, crop, ymin, cnt, coeff, ksize, lut);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

}  // namespace lavie
