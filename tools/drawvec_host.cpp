// drawvec_host.cpp -- the overlay's host/device code (csrc/dsvg_drawvec.h: the line walk and the rule that settles who wins a pixel)
// on the CPU, for a sanitizer: reads the cases tools/drawvec_dump.py wrote -- the synthetic tables of tests/test_gpu_drawinfo.py, the
// extreme vectors included, with the result of the sequential definition tests/_drawinfo.py --, draws each as k_drawinfo.hip does
// (marks of every block first, then the vectors, here in DESCENDING block order: the order must not matter) over a plane allocated at
// its exact size, and compares.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I digital-subband-video-1_amd/csrc tools/drawvec_host.cpp -o drawvec_host
//   python tools/drawvec_dump.py cases.bin && ./drawvec_host cases.bin
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "dsvg_drawvec.h"

struct Blk { int16_t x, y; uint8_t mode, submask, stable, reserved; };      // dsv1_blockinfo

static void marks(uint8_t *luma, const dsvg_drawgeo &G, const Blk *mv, const uint8_t *stable, int b)
{
    const int x = (b % G.nbh) * G.bw, y = (b / G.nbh) * G.bh;
    for (int i = x; i < x + G.bw && i < G.w; i++) luma[(size_t)y * G.stride + i] = 0;
    for (int k = y; k < y + G.bh && k < G.h; k++) luma[(size_t)k * G.stride + x] = 0;
    if ((G.mode & 1) && (stable[b] & 1)) {
        const int a = x + G.bw / 2, r = y + G.bh / 2, q = G.bw / 4;
        for (int k = -q; k <= q; k++)
            if (r < G.h && a + k >= 0 && a + k < G.w) luma[(size_t)r * G.stride + a + k] = (uint8_t)((k & 1) * 255);
    }
    if ((G.mode & 4) && mv[b].mode == 1)
        for (int t = 0; t < 4; t++)
            if ((mv[b].submask >> t) & 1) {
                const int a = dsvg_dot_x(x, G.bw, t), r = dsvg_dot_y(y, G.bh, t);
                if (a < G.w && r < G.h) luma[(size_t)r * G.stride + a] = 255;
            }
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int ncases = 0, bad = 0;
    int32_t hd[6];
    while (fread(hd, sizeof(hd), 1, f) == 1) {
        dsvg_drawgeo G;
        G.w = hd[0]; G.h = hd[1]; G.stride = hd[0]; G.bw = hd[2]; G.bh = hd[3]; G.mode = hd[4];
        G.nbh = (G.w + G.bw - 1) / G.bw; G.nbv = (G.h + G.bh - 1) / G.bh;
        const int n = hd[5], nblk = G.nbh * G.nbv;
        const size_t px = (size_t)G.w * G.h;
        std::vector<Blk> tab((size_t)n * nblk);
        std::vector<uint8_t> in(px * n), want(px * n);
        if (fread(tab.data(), sizeof(Blk), tab.size(), f) != tab.size() || fread(in.data(), 1, in.size(), f) != in.size() ||
            fread(want.data(), 1, want.size(), f) != want.size()) { fprintf(stderr, "short case\n"); return 2; }
        for (int p = 0; p < n; p++) {
            std::vector<uint8_t> luma(in.begin() + px * p, in.begin() + px * (p + 1));      // exactly the plane: a store outside it is caught
            const Blk *mv = tab.data() + (size_t)p * nblk;
            std::vector<uint8_t> stable(nblk);
            for (int b = 0; b < nblk; b++) stable[b] = mv[b].stable;
            for (int b = 0; b < nblk; b++) marks(luma.data(), G, mv, stable.data(), b);
            if (G.mode & 2)
                for (int b = nblk - 1; b >= 0; b--)
                    if (mv[b].mode == 0) dsvg_draw_vector(luma.data(), G, mv, stable.data(), b);
            if (memcmp(luma.data(), want.data() + px * p, px)) {
                size_t i = 0;
                while (luma[i] == want[px * p + i]) i++;
                fprintf(stderr, "%dx%d blocks %dx%d mode %d picture %d: differs at (%zu, %zu): %d, the definition has %d\n", G.w, G.h, G.bw, G.bh,
                        G.mode, p, i % G.w, i / G.w, luma[i], want[px * p + i]);
                bad++;
            }
        }
        ncases++;
    }
    fclose(f);
    printf("%d cases, %d pictures differ\n", ncases, bad);
    return bad || !ncases ? 1 : 0;
}
