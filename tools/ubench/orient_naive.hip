// The yardstick tools/orient_cost.py times k_orient_tr against: ROT90 of tightly packed planar 8-bit frames by a deliberately plain
// kernel -- one byte per lane, lanes along the INPUT rows (coalesced byte loads), every byte stored on its own at its rotated place
// (consecutive lanes store one output row apart), no LDS, no vector access.  Same frames, same planes, same result as the library's
// pass; it exists only to be measured.
// build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o liborient_naive.so orient_naive.hip ; tools/orient_cost.py loads it (and
// builds it where it is missing).
#include <hip/hip_runtime.h>
#include <cstdint>

// one plane of every frame: O[y][x] = I[IH-1-x][y], O of IW rows of IH samples
__global__ __launch_bounds__(256) void k_rot90_naive(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int IW, int IH, long long off, long long fb)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)IW * IH) return;
    const int r = (int)(i / IW), c = (int)(i - (long long)r * IW);           // the input sample
    const long long base = (long long)blockIdx.y * fb + off;
    dst[base + (long long)c * IH + (IH - 1 - r)] = src[base + i];
}

// nframes frames of w x h at chroma shifts (hs, vs), hs == vs; frames in [1, 65535]
extern "C" int orient_naive_rot90(void *stream, const void *src, void *dst, int w, int h, int hs, int vs, int nframes)
{
    if (!src || !dst || w < 1 || h < 1 || hs != vs || nframes < 1 || nframes > 65535) return -1;
    const int cw = (w + (1 << hs) - 1) >> hs, ch = (h + (1 << vs) - 1) >> vs;
    const long long fb = (long long)w * h + 2LL * cw * ch;
    long long off = 0;
    for (int k = 0; k < 3; k++) {
        const int pw = k ? cw : w, ph = k ? ch : h;
        const long long blocks = ((long long)pw * ph + 255) / 256;
        if (blocks > 0x7fffffffLL) return -1;
        hipLaunchKernelGGL(k_rot90_naive, dim3((unsigned)blocks, nframes), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)src, (uint8_t *)dst, pw, ph,
                           off, fb);
        off += (long long)pw * ph;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
