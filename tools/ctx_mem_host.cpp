// ctx_mem_host.cpp -- the plan of a context's memory (csrc/dsvg_ctx_mem.h: plan_ctx_mem, ctx_mem_grow, ctx_scan_layout) on the CPU, for a
// sanitizer: three geometries whose CtxMemGeo is written out by hand (from the frame, coefficient and scan layouts of those pictures),
// the rows into an array of exactly the rows the plan has, every lazy id through ctx_mem_grow.  It prints what tools/ctx_mem_dump.py
// --raw prints from the library's queries for the same three: the two outputs must be equal.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I digital-subband-video-1_amd/csrc tools/ctx_mem_host.cpp -o ctx_mem_host
//   ./ctx_mem_host > a.txt && python tools/ctx_mem_dump.py --raw > b.txt && cmp a.txt b.txt
#include <stdio.h>
#include <memory>
#include "dsvg_ctx_mem.h"

struct Case { const char *args; CtxMemGeo g; };
static const Case CASES[] = {
    // levels, pitch, total, s3total, s1total, s5total, ll, nz_total, bits_per_job, chunks_per_job, nblk, n_src, n_recon, max_jobs, out_slots, nwin, rc_slots,
    // mc_fused, sizeof HzChunkSum, HzPlaneSum, DMV, JobDev, RcJobDev, dsvg_rc_state, HzParseChunk
    { "96 64 5 0 2 3 2 4 0 0", { 3, {99328, 74240, 62208, 57600}, 9216, 144, 2304, 16, {96, 24, 24}, 10240, 19200, 5, 24, 2, 3, 2, 4, 3, 3, 1, 48, 32, 12, 2040, 16, 64, 24 } },
    { "250 130 4 2 24 24 16 48 0 0", { 2, {231168, 123648, 82432}, 65260, 1088, 16320, 80, {544, 272, 272}, 71680, 131328, 35, 144, 24, 24, 16, 48, 4, 24, 1, 48, 32, 12, 2040, 16, 64, 24 } },
    { "1920 1080 5 1 1 192 64 64 0 0", { 1, {3927552, 1210880}, 3110400, 48720, 777600, 3064, {32400, 8160, 8160}, 3115008, 6221568, 1521, 690, 1, 192, 64, 64, 2, 192, 1, 48, 32, 12, 2040, 16, 64, 24 } },
};
static const size_t NEEDS[] = {1, 4095, 196672, ((size_t)1 << 20) + 1, (size_t)64 << 20};

int main()
{
    for (const Case &c : CASES) {
        dsvg_ctx_mem_row probe[CM_N_CREATE];
        size_t totals[2];
        const int n = plan_ctx_mem(c.g, probe, totals);
        std::unique_ptr<dsvg_ctx_mem_row[]> rows(new dsvg_ctx_mem_row[n]);           // exactly the plan's rows: a row too many is the sanitizer's
        if (plan_ctx_mem(c.g, rows.get(), nullptr) != n) return 1;
        printf("ctx %s: %d rows, device %zu, pinned %zu\n", c.args, n, totals[0], totals[1]);
        for (int i = 0; i < n; i++) {
            const dsvg_ctx_mem_row &r = rows[i];
            printf("%s %d %zu %zu %zu %d %zu\n", ctx_mem_name(r.id), r.kind, r.count, r.size, r.pad, r.zeroed, r.bytes);
        }
        for (int id = CM_N_CREATE; id < CM_N; id++)
            for (size_t need : NEEDS)
                for (int few = 0; few < 2; few++)
                    printf("%s need %zu few %d: %zu %zu\n", ctx_mem_name(id), need, few, ctx_mem_lazy_bytes(id, c.g, ctx_mem_grow(id, c.g, need, 0, few != 0)),
                           ctx_mem_lazy_bytes(id, c.g, ctx_mem_grow(id, c.g, need, 4096, few != 0)));
    }
    // the scan bookkeeping of the first case: 96x64 4:2:0, planes of 3 + 1 + 1 chunks
    CtxScan S;
    const int nchunks[3] = {3, 1, 1}, cw[3] = {96, 48, 48}, ch[3] = {64, 32, 32};
    ctx_scan_layout(S, nchunks, cw, ch, CASES[0].g.ll);
    return S.nz_total == CASES[0].g.nz_total && S.bits_per_job == CASES[0].g.bits_per_job && S.chunks_per_job == CASES[0].g.chunks_per_job ? 0 : 1;
}
