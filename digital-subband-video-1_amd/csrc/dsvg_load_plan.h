// dsvg_load_plan.h -- what a source load (dsvg_load_frames, _strided, _map, _map_ex: load_core in dsvg_pipe.hip) decides on the host before it
// launches anything: plain C++17 without a HIP include or a context, so that the device-free query dsvg_load_plan can ask it about any
// geometry, alignment and switch.  plan_load reads LoadGeo and the call's own facts and writes dsvg_load_plan_out (include/dsvg.h); load_core
// launches from the plan and decides nothing itself.  The kernels' side of the same decisions is in k_frame.hip: k_unpack picks its body
// per plane from the plane's width, the address it is given and the pyramid slabs it is handed, launch_extend picks k_extend16 for
// planes a multiple of 16 wide; the plan states what they will pick, and the profiler's launch counts hold them to it on a device
// (tests/test_gpu_load_paths.py).
#ifndef DSVG_LOAD_PLAN_H
#define DSVG_LOAD_PLAN_H

#include <string.h>
#include <algorithm>
#include "../../include/dsvg.h"

// the integers of a context the decisions read (load_geo in dsvg_pipe.hip derives them, for a context and for the query alike)
struct LoadGeo {
    int levels;                                              // pyramid levels above level 0
    int w[DSVG_MAX_PYRAMID + 1], h[DSVG_MAX_PYRAMID + 1];    // the luma plane of every level
    int cw, ch;                                              // a chroma plane of level 0
    bool c_alike;                                            // both chroma planes of level 0 alike in size and stride
    // level l: the slab's base, a slot's pitch and the stride and offset of the luma plane (level 0: of all three planes) are multiples of 16
    bool lay16[DSVG_MAX_PYRAMID + 1];
    bool l2_dword;                                           // level 2: stride, offset and pitch are multiples of 4
    bool sum_dword;                                          // the top level: the luma plane's stride and every slot's first pixel are dword aligned
    int ring_x16, ring_y4;                                   // a luma-in-place frame's ring: 16-pixel columns / 4-row groups in from each edge
};

// DSV1_NO_UNPACK_SIDES, DSV1_NO_LEVEL_SIDES, DSV1_NO_FUSE_LEVEL2 (A/B): read from the environment by dsvg_pipe.hip, once per process;
// plan_load takes them as an argument, so a caller can ask it about any setting
struct LoadSwitches { bool no_unpack_sides, no_level_sides, no_fuse_level2; };

enum { LOAD_K_UNPACK = 0, LOAD_K_EXTEND = 1, LOAD_K_EXTEND16 = 2, LOAD_K_DS2X = 3, LOAD_K_LUMA_SUM = 4 };      // dsvg_load_plan_out.launches / .bytes

// k_unpack with the first pyramid level fused in: 16 pixels and two rows per thread, no border pixel enters a 2x2 mean
static inline bool load_fuses_level1(const LoadGeo &G) { return (G.w[0] & 15) == 0 && (G.h[0] & 1) == 0; }
// ... and the second one too: four source rows per thread, both levels exact halvings
static inline bool load_fuses_level2(const LoadGeo &G)
{
    return load_fuses_level1(G) && (G.h[0] & 3) == 0 && G.w[1] * 2 == G.w[0] && G.h[1] * 2 == G.h[0] && G.w[2] * 4 == G.w[0] && G.h[2] * 4 == G.h[0] && G.l2_dword;
}
// can the kernel that writes a level's luma rows (k_ds2x, or k_unpack for a fused level) write their side borders too?
static inline bool load_level_sides_ok(const LoadGeo &G, int l) { return (G.w[l] % 16) == 0 && G.lay16[l]; }
// chroma in place: the forward transforms read whole 8-byte patch rows and never leave the picture when the chroma planes are even
// (no extra coefficient column: frame.c:39-42) and a multiple of 8 wide; both chroma planes alike
static inline bool load_chroma_in_place_geo(const LoadGeo &G) { return (G.cw % 8) == 0 && (G.ch % 2) == 0 && G.c_alike; }
// luma in place: the geometry must take k_unpack's fused pyramid levels 1 and 2 (the bordered copy is then read by the level-0 motion
// search alone), and the ring must leave an interior worth the trouble
static inline bool load_luma_in_place_geo(const LoadGeo &G)
{
    return load_chroma_in_place_geo(G) && G.levels >= 2 && (G.w[0] % 16) == 0 && (G.h[0] % 4) == 0 && load_fuses_level1(G) && load_fuses_level2(G) &&
           2 * 16 * G.ring_x16 + 64 <= G.w[0] && 2 * 4 * G.ring_y4 + 64 <= G.h[0] && G.ring_x16 < 256 && G.ring_y4 < 256;
}

// The plan of one load of n frames.  src_mod16 / pitch_mod16: the source pointer / the distance between two frames modulo 16;
// n_chroma_in_place, n_luma_in_place: the frames of the call whose slot-table entry carries bit 30 / bit 29.  Writes P alone.
static inline void plan_load(const LoadGeo &G, const LoadSwitches &sw, bool with_pyramid, int src_mod16, int pitch_mod16, int n, int n_chroma_in_place,
                             int n_luma_in_place, dsvg_load_plan_out &P)
{
    memset(&P, 0, sizeof(P));
    const int w0 = G.w[0], h0 = G.h[0], n_chroma = n - n_chroma_in_place;
    const bool aligned = src_mod16 == 0 && pitch_mod16 == 0;
    P.levels = G.levels;
    P.ring_x16 = G.ring_x16; P.ring_y4 = G.ring_y4;
    P.chroma_in_place_ok = load_chroma_in_place_geo(G); P.luma_in_place_ok = load_luma_in_place_geo(G);
    // the first pyramid level comes out of the unpack kernel when the luma plane allows it (one read of the frame less); the kernel's
    // fused path needs 16-byte aligned frames: a caller's odd device pointer takes the separate passes
    P.fuse1 = with_pyramid && G.levels >= 1 && load_fuses_level1(G) && aligned;
    // k_unpack writes the 64-byte side borders of every row (and k_extend16 is told tb_only): every plane on a 16-byte path of both
    P.sides = aligned && G.lay16[0] && ((size_t)w0 * h0 % 16) == 0 && ((size_t)G.cw * G.ch % 16) == 0 && (w0 % 16) == 0 && (G.cw % 16) == 0 && !sw.no_unpack_sides;
    // the pyramid levels whose width allows it get their side borders from the kernel that writes their rows as well
    P.sides1 = P.fuse1 && P.sides && !sw.no_level_sides && load_level_sides_ok(G, 1);
    // ... and the second level with it (one pass over level 1 less) when both are exact halvings
    P.fuse2 = P.fuse1 && !sw.no_fuse_level2 && G.levels >= 2 && load_fuses_level2(G);
    P.sides2 = P.fuse2 && P.sides && !sw.no_level_sides && load_level_sides_ok(G, 2);
    // the body k_unpack takes for each plane of the call's first frame (every frame's, where the pitch is a multiple of 16; a later
    // frame of another pitch takes the scalar or the 16-byte body as its own address falls -- neither fuses, neither writes sides)
    size_t poff = 0;
    for (int c = 0; c < 3; c++) {
        const int w = c ? G.cw : w0, h = c ? G.ch : h0;
        const bool vec = (w & 15) == 0 && ((src_mod16 + poff) & 15) == 0;
        if (c > 0 && n_chroma <= 0) P.body[c] = DSVG_UNPACK_NONE;
        else if (c == 0 && vec && P.fuse1 && P.fuse2 && (h & 3) == 0) P.body[c] = DSVG_UNPACK_FUSED2;
        else if (c == 0 && vec && P.fuse1 && (h & 1) == 0) P.body[c] = DSVG_UNPACK_FUSED1;
        else P.body[c] = vec ? DSVG_UNPACK_V16 : DSVG_UNPACK_SCALAR;
        poff += (size_t)w * h;
    }
    P.grid_planes = n_chroma > 0 ? 3 : 1;
    // algorithmic bytes of k_unpack: every copied plane read once and written once (the frames whose chroma stays in the caller's clip
    // copy none), less the interior a luma-in-place frame does not write, + the pyramid levels written
    double ring_saved = 0.0;
    if (n_luma_in_place > 0 && G.ring_x16 > 0)
        ring_saved = (double)n_luma_in_place * std::max(0, w0 - 2 * 16 * G.ring_x16) * std::max(0, h0 - 2 * 4 * G.ring_y4);
    P.launches[LOAD_K_UNPACK] = 1;
    P.bytes[LOAD_K_UNPACK] = 2.0 * ((double)n * w0 * h0 + 2.0 * n_chroma * G.cw * G.ch) - ring_saved + (P.fuse1 ? 0.25 * n * w0 * h0 : 0.0) + (P.fuse2 ? 0.0625 * n * w0 * h0 : 0.0);
    for (int l = 0; l <= (with_pyramid ? G.levels : 0); l++) {
        dsvg_load_level &o = P.level[l];
        o.w = G.w[l]; o.h = G.h[l];
        bool ls = P.sides;
        if (l > 0) {
            const bool fused = (l == 1 && P.fuse1) || (l == 2 && P.fuse2);
            ls = fused ? (l == 1 ? P.sides1 : P.sides2) : (!sw.no_level_sides && load_level_sides_ok(G, l));
            if (!fused) {
                o.ds2x = 1; o.ds2x_sides = ls;
                o.ds2x_tail = (o.w & 3) != 0; o.src_odd_w = G.w[l - 1] & 1; o.src_odd_h = G.h[l - 1] & 1;
                P.launches[LOAD_K_DS2X]++;
                P.bytes[LOAD_K_DS2X] += 5.0 * n * (double)o.w * o.h;
            }
        }
        // launch_extend: k_extend16 where every plane it covers (level 0: all three) is a multiple of 16 wide
        const bool v16 = G.lay16[l] && (o.w % 16) == 0 && (l > 0 || (G.cw % 16) == 0);
        o.border = v16 ? DSVG_BORDER_EXTEND16 : DSVG_BORDER_EXTEND;
        o.tb_only = ls;
        const int k = v16 ? LOAD_K_EXTEND16 : LOAD_K_EXTEND;
        P.launches[k]++;
        P.bytes[k] += 8.0 * ((double)(o.h + 128) * 32 + 32.0 * o.w) * n;       // dwords of the luma border
    }
    if (with_pyramid) {
        const int t = G.levels;
        P.luma_sum = 1;
        P.luma_sum_dword = (G.w[t] & 3) == 0 && G.sum_dword;
        P.launches[LOAD_K_LUMA_SUM] = 1;
        P.bytes[LOAD_K_LUMA_SUM] = 1.0 * n * (double)G.w[t] * G.h[t];
    }
}

#endif
