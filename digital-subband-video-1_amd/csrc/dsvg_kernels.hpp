// dsvg_kernels.hpp -- launcher prototypes and by-value kernel argument blocks.
#pragma once
#include "dsvg_dev.hpp"

#define DSVG_BORDER 64

struct Prof;
struct SbtGeo3 { SbtGeo g[3]; };

struct McGeo {
    int blk_w, blk_h, nbh, nbv, hs, vs;
    int w[3], h[3], stride[3];
    size_t off[3];
    int cw_extra[3];         // coefficient plane one column wider than the pixel plane
};

struct HmeArgs {
    FrameLayout L[6];        // level 0 = full frames, level i = pyramid level i
    const uint8_t *slab[6];
    const int *cur_slots, *ref_slots;
    // chroma planes of every source slot (level 0's variance test, hme.c:269-300,667-681): pixel (0,0) of U / V and the row stride --
    // the bordered frame's, or the caller's packed clip for frames loaded in place (dsvg_load_frames_map_ex)
    const unsigned long long *slot_cu, *slot_cv;
    const int *slot_cs;
    DMV *mvf;                // [pair][level][nblk]
    unsigned *aux_tex;       // [pair][nblk] block texture (for the high_detail pass)
    int *aux_var;            // [pair][nblk] centre-window variance
    // (round 5) per source slot: the frame's luma plane in the caller's packed clip (row stride = the picture's width), or 0: the level-0 search
    // reads a block's source and reference rows there when everything it can touch lies inside the picture (hme_block, `deep`) -- of the
    // bordered copies only a ring exists for such frames (k_unpack, slot-table bit 29)
    const unsigned long long *slot_y;
    int deep_r;
    // [slot][nblk][4]: sum / sum of squares of the U and of the V block of every FULL block of a source slot (k_hme_csum), or nullptr:
    // level 0's chroma variance test then fetches the blocks itself
    unsigned *csum;
    int levels, nxb, nyb, nblk, blk_w, blk_h;
};
// HmeArgs.deep_r: a level-0 vector's reach (k_hme.hip, `deep`: 2^(levels+1) - 1 full pixels) + the nine-point search, half-pel lattice, window
// slack; and the ring of a luma-in-place frame's bordered copy that the blocks nearer an edge can touch: a block and twice deep_r in from
// each edge, in 16-pixel columns / 4-row groups (k_unpack, slot-table bit 29)
static inline int hme_deep_r(int levels) { return (2 << levels) + 8; }
static inline int hme_ring_x16(int blk_w, int deep_r) { return (blk_w + 2 * deep_r + 15) / 16; }
static inline int hme_ring_y4(int blk_h, int deep_r) { return (blk_h + 2 * deep_r + 3) / 4; }

// k_sbt.hip
int  sbt_tail_supported(const SbtGeo &g);
void sbt_set_func_attributes();
bool mc_fusable(const struct McGeo &MG);
// the decisions behind the forward plan (general kernel: a mask of DSVG_FWD_*) and the motion search's (per level; csum: see
// dsvg_dispatch), as functions of the geometry alone, and where the executors note what the plans said (dsvg_dispatch_last)
int  fwd_general_mask(const SbtGeo3 &G, const struct McGeo &mc, int c0, int npl, int general_whole);
struct HmeLevelPlan { int nkbf, fullx, fully, nfull, nrest, parts; };
HmeLevelPlan hme_level_plan(const struct HmeArgs &A, int level);
int  hme_csum_plan(const struct HmeArgs &A, int *fullx, int *fully);
void dispatch_note_fwd(int group, int mask);
void dispatch_note_hme(const struct HmeArgs &A, int level, const HmeLevelPlan &P);
void dispatch_note_csum(int csum);
void dispatch_note_threads(int tail, int scan);      // the workgroup sizes the k_tail_q step / the k_hz_scan launch took (0: not this one)
// The inverse transform of planes [c0, c0+npl) of njobs pictures (all P or all I) as a pure function of the geometry, the caller's
// flags and the A/B switches: every launch in order, decided once.  launch_inv_plan runs a plan and decides nothing; the border
// question of enqueue_recon (InvPlan.fb) and the device-free query dsvg_inv_plan read the same plan.
struct InvSwitches { bool no_patch_part, no_edge_tiles, no_fused_border, no_xcd_order; };   // DSV1_NO_PATCH_PART / _EDGE_TILES / _FUSED_BORDER / _XCD_ORDER
const InvSwitches &inv_switches();                          // the process's own, read from the environment once
struct InvStep {
    int kid;                 // KID_INV_*: names the template instance
    int gx, gy, gz;          // the grid; xcd: launched as tile_grid(gx, gy, gz) and decoded with mk_xcd_grid(gx, gy, gz), plain = DSV1_NO_XCD_ORDER
    bool xcd, plain;
    int bx, by;              // the block
    size_t lds;              // dynamic LDS bytes
    int a[4];                // the kernel's trailing integer arguments: tcx, -tcy-1 | er, eb | imax, jmax, jpart, fb
    double bytes;            // the algorithmic bytes of Prof::begin
    int cover, cx, cy;       // the level-3 cells of every plane whose pixels the step writes: DSVG_INV_COVER_*
};
struct InvPlan {
    int n;
    InvStep s[5];
    int fb;                  // the chroma patch kernel writes the reconstruction's borders, of its own planes and of the luma plane (JobDev.ext)
};
InvPlan inv_sbt_plan(const SbtGeo3 &G, int njobs, int c0, int npl, int isP, int with_tail, int insym, int patch_kernel, int fuse_border, const InvSwitches &sw);
void launch_inv_plan(hipStream_t st, const JobDev *jobs, const SbtGeo3 &G, int c0, int npl, const InvPlan &P, Prof *pf);
void launch_inv_sbt(hipStream_t st, const JobDev *jobs, int njobs, const SbtGeo3 &G, int c0, int npl, int isP, Prof *pf = nullptr, int with_tail = 1,
                    int insym = 0, int patch_kernel = 0,    // patch_kernel: sparse P pictures (flags valid, prediction given): unfiltered planes take k_inv_patch_c
                    int fuse_border = 0);                   // the kernels also write the reconstruction's border (JobDev.ext) where the plan says they can (InvPlan.fb)
void launch_inv54_all(hipStream_t st, const JobDev *jobs, int njobs, const SbtGeo3 &G, Prof *pf = nullptr);   // levels 5..4 of all planes: then launch_inv_sbt(.., with_tail | 2)
InvPlan inv_tail_plan(const SbtGeo3 &G, int njobs, int c0, int npl);        // the LDS tails of planes [c0, c0+npl) of all jobs in one launch
// The forward transform of planes [c0, c0+npl) of njobs pictures (all P or all I) the same way: fwd_sbt_plan decides every launch
// of a plane group, fwd_step_plan the launches a frame step makes once for all planes and jobs (levels 4..5, then the LDS tail --
// with the LL quantiser and the inverse tail where llq); launch_fwd_plan runs a plan and decides nothing.  A step is an InvStep
// (cover unused); a: from_src | the general kernel's bxofs, byofs, bxstep, bystep | k_fwd_haar_mid<4>: the LL quantiser.
typedef InvStep FwdStep;
struct FwdPlan {
    int n;
    FwdStep s[5];
    bool report;             // a P plane group: the executor reports mask (dispatch_note_fwd)
    int mask;                // DSVG_FWD_*: where the general kernel goes; -1: motion compensation is not fused
};
struct FwdOpts {
    bool quantise;           // the kernels quantise and write symbol planes (the encoder), not int32 coefficients
    bool llq;                // own_mid4: k_fwd_haar_mid<4> quantises the LL region (JobDev.llq set by the caller)
    bool own_mid4, own_tail; // levels 4..5 / the LDS tail are this plane group's own launches, not the frame step's (fwd_step_plan)
};
// mc: motion compensation fused into the P forward transform; general_whole = 0: the caller knows that no block of these pictures
// is intra (the general kernel then only runs on the strips of the grid the geometry asks for); plain: DSV1_NO_XCD_ORDER
FwdPlan fwd_sbt_plan(const SbtGeo3 &G, int njobs, int c0, int npl, int isP, int from_src, const FwdOpts &o, const struct McGeo *mc, int general_whole, bool plain);
FwdPlan fwd_step_plan(const SbtGeo3 &G, int njobs, bool llq);
void launch_fwd_plan(hipStream_t st, const JobDev *jobs, const SbtGeo3 &G, int c0, int npl, const FwdPlan &P, Prof *pf, const struct McGeo *mc = nullptr, const DMV *mvs0 = nullptr);
void launch_fwd_sbt(hipStream_t st, const JobDev *jobs, int njobs, const SbtGeo3 &G, int c0, int npl, int isP, int from_src, const FwdOpts &o, Prof *pf = nullptr,
                    const struct McGeo *mc = nullptr, const DMV *mvs0 = nullptr, int general_whole = 1);
// k_hzcc.hip
void launch_hz_encode(hipStream_t st, const JobDev *jobs, int njobs, int job_chunks, Prof *pf = nullptr, double samples = 0,
                      int nplain = -1, int ll_chunks = 1);
void launch_hz_quant(hipStream_t st, const JobDev *jobs, int njobs, int job_chunks, Prof *pf, double samples, int nplain, int ll_chunks);
void launch_hz_pack(hipStream_t st, const JobDev *jobs, int njobs, int job_chunks, Prof *pf, double samples, int nplain, int ndense = -1);
void launch_hz_parse_scatter(hipStream_t st, JobDev *jobs, int njobs, int c, int nplanes, int max_entries, int max_chunks, Prof *pf = nullptr, bool all_sparse = false);
void launch_dec_clear(hipStream_t st, const JobDev *jobs, int njobs);                       // decoder: zero what the scatter leaves untouched
void launch_mc_patch(hipStream_t st, const JobDev *jobs, int njobs, const SbtGeo3 &G, const McGeo &MG, const DMV *mvs0, int ex0, int ey0, Prof *pf);
void launch_hz_dec_resolve(hipStream_t st, const JobDev *jobs, int njobs, int c0, int nplanes);
void launch_hz_unscatter(hipStream_t st, const JobDev *jobs, int njobs, int max_entries);   // decoder: take the scattered symbols down again
int  hz_scan_items_max();
void launch_gather_bits(hipStream_t st, const uint8_t *bits, const unsigned long long *tab, int nitems, uint8_t *dst);
// k_rc.hip: device-resident ABR -- mode 0: quantiser of jobs [d0, d0 + n) from their streams' state; mode 1: after their k_hz_scan,
// packet size -> statistics -> quantiser tables of each stream's next job (RcJobDev.next)
void launch_rc(hipStream_t st, JobDev *jobs, const RcJobDev *rcj, dsvg_rc_state *state, int d0, int n, int mode);
// k_bmc.hip
// mvs0: the jobs' vector arrays when they are contiguous (job j at mvs0 + j * nblocks), else null (JobDev.mvs is used)
void launch_mc(hipStream_t st, const JobDev *jobs, int njobs, const McGeo &G, int do_sub, Prof *pf = nullptr, const DMV *mvs0 = nullptr,
               const int *list = nullptr, int nlist = 0);   // list: only these blocks (job * nblocks + block)
// k_frame.hip
void launch_unpack(hipStream_t st, const uint8_t *yuv, size_t yuv_pitch, uint8_t *slab, const FrameLayout &L, int first, int n, Prof *pf = nullptr, const int *slot_tab = nullptr,
                   uint8_t *slab1 = nullptr, const FrameLayout *L1 = nullptr, bool sides = false, bool sides1 = false,
                   uint8_t *slab2 = nullptr, const FrameLayout *L2 = nullptr, bool sides2 = false, int n_chroma = -1,
                   int ring_x16 = 0, int ring_y4 = 0, int n_ring = 0);    // slot-table entries with bit 29: only the luma plane's outer ring_x16 x 16 columns / ring_y4 x 4 rows are copied
void launch_pack(hipStream_t st, uint8_t *yuv, const uint8_t *frame, const FrameLayout &L);
void launch_pack_n(hipStream_t st, uint8_t *yuv, size_t out_pitch, const uint8_t *slab, const FrameLayout &L, const int *slot_tab, int n, Prof *pf = nullptr);
void launch_extend(hipStream_t st, uint8_t *slab, const FrameLayout &L, int first, int n, int nplanes, const int *slot_tab, Prof *pf = nullptr, const JobDev *jobs = nullptr, bool tb_only = false);
void launch_ds2x(hipStream_t st, const uint8_t *sslab, const FrameLayout &SL, uint8_t *dslab, const FrameLayout &DL, int first, int n, Prof *pf = nullptr, const int *slot_tab = nullptr, bool sides = false);
void launch_luma_sum(hipStream_t st, const uint8_t *slab, const FrameLayout &L, int first, int n, unsigned *sums, Prof *pf = nullptr, const int *slot_tab = nullptr);
void launch_frame_add(hipStream_t st, uint8_t *dst, const FrameLayout &DL, const uint8_t *src, const FrameLayout &SL);
// k_quality.hip: per-plane sum of squared errors source vs reconstruction of every job, added into sse[3 * out slot + plane]
// (the out slot found from JobDev.psum = psum0 + 3 * out slot); one launch per frame step and coding stream, after its reconstruction
void launch_sse(hipStream_t st, const JobDev *jobs, int njobs, const FrameLayout &L, const HzPlaneSum *psum0, unsigned long long *sse);
// the same jobs' per-plane SSIM (8x8 windows at stride 4, fixed point: sum of rint(2^32 s)) added into ssim[3 * out slot + plane];
// sse != nullptr: the sums of squared errors too, in the same pass (k_sse's figures: launch one or the other)
void launch_ssim(hipStream_t st, const JobDev *jobs, int njobs, const FrameLayout &L, const HzPlaneSum *psum0, unsigned long long *ssim,
                 unsigned long long *sse);
// source-resolution quality (dsvg_ctx_xres_enable): every job's reconstruction upscaled to the reference geometry (dsv1_resample_*
// tables) and compared with the reference frame of its out slot (xref[out slot], nullptr: not measured), per-plane SSE and SSIM_FX
// added into xsse / xssim[3 * out slot + plane] (either may be nullptr); same launch point as launch_sse / launch_ssim
struct XresPlane {               // one plane: reconstruction sw x sh -> reference dw x dh, tables in device memory
    int sw, sh, dw, dh;
    int th, tv, tx, tile0;       // taps per axis, tiles across, first tile of the plane in blockIdx.x
    long long doff;              // plane offset inside a packed reference frame
    const int *hs;
    const short *hq;
    const int *vs;
    const short *vq;
};
struct XresGeo {
    XresPlane *planes_d = nullptr;   // [3] + tables, one allocation
    int ntiles = 0, rows_cap = 0, th_cap = 0, tv_cap = 0, span_cap = 0;
    size_t lds = 0, rfb = 0;         // LDS of a workgroup; bytes of a packed reference frame
    int rw = 0, rh = 0, filter = -1;
};
int xres_geo_build(XresGeo &G, const FrameLayout &L, int rw, int rh, int filter);   // replaces G's tables only on success
void xres_geo_free(XresGeo &G);
void launch_xres(hipStream_t st, const JobDev *jobs, int njobs, const FrameLayout &L, const XresGeo &G, const uint8_t *const *xref,
                 const HzPlaneSum *psum0, unsigned long long *xsse, unsigned long long *xssim);
// k_scale.hip: one geometry of the exact integer resampler (tables of dsv1_resample_weights in device memory, the tile height and the
// exact LDS bound chosen from them), and its entry that reads reconstruction slots for the decoders' output pass: entry i of the
// (slot, output frame) pairs tab_d reads the bordered frame at slab + slot * sfb and writes packed planar frame dst + frame * dfb
struct ScalePlane;
struct ScaleGeo {
    ScalePlane *planes_d = nullptr;      // [3] + tables, one allocation
    int ntiles = 0;
    size_t lds = 0;
    int th_tile = 0, rows_cap = 0, th_cap = 0, tv_cap = 0, span_cap = 0;
    size_t dfb = 0, sbytes = 0;          // bytes of a packed destination frame; sample bytes of a source frame
};
int  scale_geo_build(ScaleGeo &G, const FrameLayout &L, int fmt, int dw, int dh, int filter);   // source: frames of layout L; replaces G's tables only on success
void scale_geo_free(ScaleGeo &G);
void launch_scale_slots(hipStream_t st, const ScaleGeo &G, const uint8_t *slab, size_t sfb, const int *tab_d, int n, uint8_t *dst, size_t dfb, Prof *pf = nullptr);
// k_drawinfo.hip: the decoders' debug overlay (mode: DSV_DRAW_* bits, non-zero) onto the luma planes of n pictures -- picture i at
// luma0 + i * pic_pitch, w x h at row stride `stride` -- from their block tables, picture i at mvs + i * nblk and stable + i * nblk
// (nblk = ceil(w / bw) * ceil(h / bh)); two launches in stream order, every store inside the plane
void launch_drawinfo(hipStream_t st, uint8_t *luma0, size_t pic_pitch, int w, int h, int stride, int bw, int bh, int mode,
                     const DMV *mvs, const uint8_t *stable, int n);
// k_hme.hip: the motion search of npairs pairs as a plan of the geometry fields of HmeArgs and of whether it has the chroma table:
// k_hme_csum if any, the one or two k_hme_level launches of every level from the top down, k_hme_detail.  launch_hme_plan runs it.
struct HmeStep {
    int kid;                         // KID_HME_*
    int l0, nkbf, part;              // k_hme_level<L0, NKBF, PART>
    int level, cnt;                  // the level and its blocks per pair in this launch (nfull / nrest / nvx * nvy)
    int fullx, fully;                // k_hme_level, k_hme_csum
    unsigned inv_per, inv_row;       // min(floor(2^32 / d), 2^32 - 1) of cnt and of the row length the block index is split by
    int gx, gy, bx;                  // the grid (k_hme_level: gx workgroups, launched as xcd_grid(gx)) and the block
    double bytes;                    // the algorithmic bytes of Prof::begin (0 where cont)
    bool cont;                       // no bracket of its own: the launch continues the previous step's (level 0's PART 2)
};
struct HmePlan {
    int n;
    HmeStep s[2 * 6 + 2];            // (six levels, as HmeArgs.L)
    int levels, csum;                // what the executor reports (dispatch_note_*), with lv[0..levels]
    HmeLevelPlan lv[6];
};
HmePlan hme_plan(const HmeArgs &A, int npairs, bool table);
void launch_hme_plan(hipStream_t st, const HmeArgs &A, int npairs, const HmePlan &P, Prof *pf = nullptr);
void launch_hme(hipStream_t st, const HmeArgs &A, int npairs, Prof *pf = nullptr);
