"""A context's creation-time buffers, restated from their consumers' side: per buffer the element count that the kernels and copies
which index it need, with the kernel or struct that fixes the extent.  tests/test_ctx_mem_host.py holds the library's
dsvg_ctx_mem_plan (csrc/dsvg_ctx_mem.h) to it; nothing here reads that header.

Geometry comes from the existing restatements: load_plan.plane_layout (frame layout), fwd_plan.block_dims / pyramid_levels /
plane_dims (blocks, pyramid depth, coefficient planes), hz_plan.geometry (scan chunks)."""
import fwd_plan as FP
import hz_plan as HZ
import load_plan as LP

DEVICE, PINNED, SLAB = "device", "pinned", "slab"
GUARD = 256 * 1024                    # dsvg_host.hpp GUARD_BYTES: zeroed, in front of and behind a slab (Slab::alloc)
PAD = {DEVICE: 256, PINNED: 64, SLAB: 4096 + 2 * GUARD}     # behind a device buffer, a pinned one; a slab's slack and its two guards
HZ_CHUNK = 2048                       # dsvg_dev.hpp

# sizeof the device structs (csrc/dsvg_dev.hpp, include/dsvg_rc.h), counted from their definitions
SIZEOF = {
    "HzChunkSum": 48,     # 4 int + unsigned = 20, padded to 24 for the 64-bit bit_off, + 8 + 4 int
    "HzPlaneSum": 32,     # static_assert in dsvg_dev.hpp: travels to the host as 32-byte records
    "DMV": 12,            # static_assert: == DSV_MV
    "JobDev": 2040,       # dsvg_dev.hpp: the job record the kernels take by pointer
    "RcJobDev": 16,       # 4 int
    "dsvg_rc_state": 64,  # include/dsvg_rc.h
}

rsu = lambda x, s: (x + (1 << s) - 1) >> s
r8 = lambda n: (n + 7) & ~7
r4 = lambda n: (n + 3) & ~3


def frame_pitch(w, h, fmt):
    """distance of two frames in a slab: the three bordered planes back to back (frame.c:63-120), rounded up to 256"""
    hs, vs = (fmt >> 2) & 3, fmt & 3
    return (LP.plane_layout(w, h)[1] + 2 * LP.plane_layout(rsu(w, hs), rsu(h, vs))[1] + 255) & ~255


def accepted(w, h, fmt, n_src, n_recon, max_jobs, bw, bh):
    """0, or the code dsvg_ctx_create_blk refuses these arguments with (-2 argument, -3 unsupported), in the order of its checks"""
    if (bw or bh) and (not 16 <= bw <= 64 or not 16 <= bh <= 64 or bw & 3 or bh & 3):
        return -2
    if w < 32 or h < 32 or n_src < 1 or n_recon < 1 or max_jobs < 1 or fmt not in (0x0, 0x4, 0x5, 0x8):
        return -2
    if (w | h) & 1:
        return -3
    return 0


def plan(w, h, fmt, pyramid=0, n_src=1, n_recon=1, max_jobs=1, out_slots=1, bw=0, bh=0):
    """[(name, kind, count, size, zeroed)] in the order of allocation"""
    if not bw:
        bw, bh, nbh, nbv = FP.block_dims(w, h)
    else:
        nbh, nbv = (w + bw - 1) // bw, (h + bh - 1) // bh
    nblk = nbh * nbv
    levels = min(pyramid, FP.MAX_PYRAMID) if pyramid > 0 else FP.pyramid_levels(w, h, nbh, nbv)
    planes = [(W, H) for _, _, W, H in FP.plane_dims(w, h, fmt)]          # coefficient planes
    hs, vs = (fmt >> 2) & 3, fmt & 3
    fused = (bw >> hs) % 8 == 0 and (bh >> vs) % 8 == 0 and bw % 8 == 0 and bh % 8 == 0      # mc_fusable (fwd_plan.fusable, any block size)
    J, O = max_jobs, max(out_slots, max_jobs)            # a coding call fills up to max_jobs out slots (batch_geo)
    # the jobs of nwin calls in flight have host-side records of their own (code_batch_impl: win * max_jobs + j)
    SO = max(J * ((O + J - 1) // J + 1), O)
    coef = sum(W * H for W, H in planes)                                  # JobDev.coef: the planes back to back
    s3 = sum(r4(rsu(W, 3) * rsu(H, 3)) for W, H in planes)                # LL3 / LL1 / LL5 scratch: each plane's band on 16 bytes
    s1 = sum(r4(rsu(W, 1) * rsu(H, 1)) for W, H in planes)
    s5 = sum(r4(rsu(W, 5) * rsu(H, 5)) for W, H in planes)
    chunks = sum(HZ.geometry(W, H)[2] for W, H in planes)                 # k_hz_*: a chunk summary per HZ_CHUNK scan cells
    nz = chunks * HZ_CHUNK                                                # a slot per scan cell of every chunk
    ll = sum(r8(rsu(W, 3) * rsu(H, 3)) for W, H in planes)                # k_hz_collect*: 16-byte reads of the LL symbols
    bits = sum(((W * H * 2 + 255) & ~255) + 256 for W, H in planes)       # k_hz_emit: 16 bits per coefficient, on 256 bytes, 256 apart
    S = SIZEOF
    rows = [("src%d" % l, SLAB, n_src, frame_pitch(rsu(w, l), rsu(h, l), fmt), True) for l in range(levels + 1)]     # k_unpack, k_ds2x: a frame per slot and level
    rows += [
        ("recon", SLAB, n_recon, frame_pitch(w, h, fmt), True),           # JobDev.recon / ref
        ("xf", SLAB, J, frame_pitch(w, h, fmt), True),                    # JobDev.xf: a work frame per job
        ("pred", SLAB, J, frame_pitch(w, h, fmt), True),                  # JobDev.pred
        ("coef", DEVICE, coef * J, 4, True), ("s3", DEVICE, s3 * J, 4, True), ("s1", DEVICE, s1 * J, 4, True), ("s5", DEVICE, s5 * J, 4, True),
        ("nzpos", DEVICE, nz * J, 4, False), ("nzval", DEVICE, nz * J, 4, False),       # k_hz_collect writes before k_hz_emit reads
        ("chunks", DEVICE, chunks * J, S["HzChunkSum"], True),
        ("sym", DEVICE, nz * J, 2, True),                                 # int16 symbol per scan cell
        ("nzf", DEVICE, (nz >> 2) * J, 1, True),                          # a flag byte per 4 scan cells
        ("symP", DEVICE, nz * J, 2, True),
        ("pflag", DEVICE, s3 * J, 1, True),                               # a flag byte per 8x8 patch, indexed like s3
        ("cflag", DEVICE, chunks * J, 1, True),                           # a flag byte per chunk
        ("llsym", DEVICE, ll * J, 4, True),
        ("stat", DEVICE, 8 * 64, 4, True),                                # [4][64] sharded tile counters, twice (dsvg_ctx_tile_stats2)
        ("psum", DEVICE, 3 * O, S["HzPlaneSum"], True),                   # k_hz_scan: a summary per plane and out slot
        ("bits", DEVICE, bits * O, 1, True),
        ("mvs", DEVICE, nblk * O, S["DMV"], True), ("stable", DEVICE, nblk * O, 1, True),      # JobDev.mvs / stable: per block
        ("jobs_d", DEVICE, O, S["JobDev"], True),
        ("rc_state_d", DEVICE, max(n_recon, J), S["dsvg_rc_state"], True),      # k_rc: a state per stream (batch_geo: rc_slots)
        ("rcj_d", DEVICE, O, S["RcJobDev"], True), ("rcj_h", PINNED, SO, S["RcJobDev"], True),
        ("mvf", DEVICE, (levels + 1) * nblk * O, S["DMV"], True),         # k_hme_level: a field per pyramid level and pair
        ("aux_tex", DEVICE, nblk * O, 4, True), ("aux_var", DEVICE, nblk * O, 4, True),
        ("csum", DEVICE, nblk * 4 * n_src, 4, True),                      # k_hme_csum: [n_src][nblk][4]
        ("slots_d", DEVICE, 3 * O, 4, True),                              # cur, ref, recon tables
        ("luma_sums", DEVICE, n_src, 4, True),                            # k_luma_sum
        ("jobs_h", PINNED, SO, S["JobDev"], True),
        ("gtab_d", DEVICE, 9 * O, 8, True), ("gtab_h", PINNED, 9 * O, 8, True),         # k_gather_bits: 3 words per plane payload
        ("psum_h", PINNED, 3 * O, S["HzPlaneSum"], True),
        ("mv_h", PINNED, nblk * SO, S["DMV"], True), ("stable_h", PINNED, nblk * SO, 1, True),
        ("slots_h", PINNED, 3 * SO, 4, True), ("luma_h", PINNED, n_src, 4, True),
        ("aslots_h", PINNED, 2 * O, 4, True), ("amv_h", PINNED, nblk * O, S["DMV"], True),
    ]
    if fused:           # k_mc_patch's intra list: a block index per block of every job record
        rows += [("ilist_h", PINNED, nblk * SO, 4, True), ("ilist_d", DEVICE, nblk * SO, 4, False)]
    # HmeArgs.slot_cu / slot_cv / slot_cs / slot_y: a pointer or stride per source slot; 64 bytes behind each, device side too
    rows += [("slot_cu_h", PINNED, n_src, 8, False), ("slot_cv_h", PINNED, n_src, 8, False), ("slot_cs_h", PINNED, n_src, 4, False),
             ("slot_cu_d", DEVICE, n_src, 8, False), ("slot_cv_d", DEVICE, n_src, 8, False), ("slot_cs_d", DEVICE, n_src, 4, False),
             ("slot_y_h", PINNED, n_src, 8, True), ("slot_y_d", DEVICE, n_src, 8, True)]
    return rows


def pad_of(name, kind):
    return 64 if name.startswith("slot_") else PAD[kind]


# lazy buffers: name -> (kind, element size, pad, rule(need, geometry dict) -> capacity in elements once need exceeds what is held)
MIB = 1 << 20


def lazy_rules(g, few=False):
    """g: dict(n_src, n_recon, max_jobs, out_slots (raised), pitch0)"""
    fixed = lambda n: (lambda need: max(n, need))
    asked = lambda need: need
    R = {
        "ltab_d": (DEVICE, 4, 64, fixed(g["n_src"])),
        "yuv_stage": (DEVICE, 1, 256, asked), "ingest0": (DEVICE, 1, 256, asked), "ingest1": (DEVICE, 1, 256, asked),
        "gath_d": (DEVICE, 1, 0, (lambda need: max(MIB, need)) if few else (lambda need: 2 * max(need - 64, 0) + MIB)),
        "xref_d": (DEVICE, 8, 256, fixed(g["out_slots"])), "xref_h": (PINNED, 8, 64, fixed(g["out_slots"])),
        "otab_d": (DEVICE, 4, 64, fixed(2 * g["n_recon"])), "osc_tab_d": (DEVICE, 4, 64, fixed(2 * g["n_recon"])),
        "osc_scratch": (DEVICE, 1, 256, asked),
        "dec_h0": (PINNED, 1, 0, lambda need: 2 * need + MIB), "dec_d0": (DEVICE, 1, 256, lambda need: 2 * need + MIB),
        "dec_meta": (DEVICE, 24, 0, lambda need: 2 * need + 4096),            # HzParseChunk: two 64-bit masks, two ints
        "dec_flag_d": (DEVICE, 4, 0, fixed(2 * g["max_jobs"])), "dec_flag_h": (PINNED, 4, 0, fixed(2 * g["max_jobs"])),
        "draw_scratch": (DEVICE, 1, 256, fixed(g["pitch0"] * g["max_jobs"])),
    }
    R["gath_h"] = (PINNED,) + R["gath_d"][1:]
    R["dec_h1"], R["dec_d1"] = R["dec_h0"], R["dec_d0"]
    for k in range(4):
        R["q%d_dev" % k] = (DEVICE, 8, 256, fixed(3 * g["out_slots"]))
        R["q%d_host" % k] = (PINNED, 8, 64, fixed(3 * g["out_slots"]))
    return R


def grow_bytes(name, g, need, cap, few=False):
    kind, size, pad, rule = lazy_rules(g, few)[name]
    n = cap if need <= cap else max(rule(need), need)
    return n * size + pad
