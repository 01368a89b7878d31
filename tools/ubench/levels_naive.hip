// The yardstick tools/levels_cost.py times k_levels and k_histogram against: the same two jobs by deliberately plain kernels -- one byte
// per lane, the tables read from global memory ([3][256] bytes, as the caller holds them), the histogram counted with one global atomic
// per sample straight into [n][3][256]; no LDS, no vector access, no privatisation.  Same frames, same planes, same results as the
// library's passes; they exist only to be measured.
// build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o liblevels_naive.so levels_naive.hip ; tools/levels_cost.py loads it (and
// builds it where it is missing).
#include <hip/hip_runtime.h>
#include <cstdint>

// a frame: luma in [0, e0), U in [e0, e1), V in [e1, fb)
__global__ __launch_bounds__(256) void k_levels_naive(const uint8_t *src, uint8_t *dst, const uint8_t *__restrict__ lut, long long e0, long long e1, long long fb,
                                                      long long nbytes)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nbytes) return;
    const long long r = i % fb;
    dst[i] = lut[(r < e0 ? 0 : r < e1 ? 256 : 512) + src[i]];
}

__global__ __launch_bounds__(256) void k_histogram_naive(const uint8_t *__restrict__ src, unsigned *hist, long long e0, long long e1, long long fb, long long nbytes)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nbytes) return;
    const long long f = i / fb, r = i - f * fb;
    atomicAdd(&hist[f * 768 + (r < e0 ? 0 : r < e1 ? 256 : 512) + src[i]], 1u);
}

static int geometry(int w, int h, int hs, int vs, int nframes, long long *e0, long long *e1, long long *fb, long long *blocks)
{
    if (w < 1 || h < 1 || nframes < 1) return -1;
    const long long cw = (w + (1 << hs) - 1) >> hs, ch = (h + (1 << vs) - 1) >> vs;
    *e0 = (long long)w * h; *e1 = *e0 + cw * ch; *fb = *e1 + cw * ch;
    *blocks = (*fb * nframes + 255) / 256;
    return *blocks > 0x7fffffffLL ? -1 : 0;
}

// lut: device memory, [3][256] bytes
extern "C" int levels_naive(void *stream, const void *src, void *dst, const void *lut, int w, int h, int hs, int vs, int nframes)
{
    long long e0, e1, fb, blocks;
    if (!src || !dst || !lut || geometry(w, h, hs, vs, nframes, &e0, &e1, &fb, &blocks)) return -1;
    hipLaunchKernelGGL(k_levels_naive, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)src, (uint8_t *)dst, (const uint8_t *)lut, e0, e1,
                       fb, fb * nframes);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// hist: device memory, uint32 [nframes][3][256]; zeroed on the stream first
extern "C" int histogram_naive(void *stream, const void *src, void *hist, int w, int h, int hs, int vs, int nframes)
{
    long long e0, e1, fb, blocks;
    if (!src || !hist || geometry(w, h, hs, vs, nframes, &e0, &e1, &fb, &blocks)) return -1;
    if (hipMemsetAsync(hist, 0, sizeof(unsigned) * 768 * (size_t)nframes, (hipStream_t)stream) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_histogram_naive, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)src, (unsigned *)hist, e0, e1, fb,
                       fb * nframes);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
