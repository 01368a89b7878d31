"""The product's plan for a source load (dsvg_load_frames and its siblings), stated from what the load's kernels need.

csrc/k_frame.hip's kernels fork on geometry and alignment by themselves; the host (plan_load, csrc/dsvg_load_plan.h) must hand them
pointers and flags that agree with those forks, or a border or a pyramid level is written twice or never.  This module says, for a
geometry, a source address and the three switches, what each kernel will do, from the kernel's side:

  * k_unpack copies a plane 16 bytes per lane where the plane is a multiple of 16 wide and the address of its first pixel is a multiple
    of 16, else byte by byte; the luma plane's lanes also write pyramid level 1 (two rows per lane) or levels 1 and 2 (four rows per
    lane) if they are handed those slabs -- so the host may hand them only where EVERY frame's luma takes a 16-byte lane and the rows
    come in pairs / fours; a level written there needs no k_ds2x.  Its lanes at a row's ends write the 64 border bytes beside them with
    16-byte stores (`sides`): sound only where every plane of every frame takes the 16-byte lanes and the border starts on 16 bytes.
  * k_ds2x writes a level four means per lane; the lanes at a row's ends can write the side borders if the level is a multiple of 16 wide.
  * launch_extend takes k_extend16 where every plane it covers is a multiple of 16 wide; tb_only where the level's side borders exist.
  * k_luma_sum reads dwords where the top level is a multiple of 4 wide.

It restates the product's planning, not the reference: what is right is decided by the oracle; this module only says which code a
case reaches.  tests/test_load_plan_host.py holds it against the library's own plan (dsvg_load_plan) over the whole sweep.

The decision algebra is written on numpy arrays (one entry per geometry) so that the sweep costs seconds; plan() is the same for one.
"""
import functools

import numpy as np

from fwd_plan import MAX_PYRAMID, block_dims, pyramid_levels
from inv_plan import BORDER, FORMATS, rsu

NO_UNPACK_SIDES, NO_LEVEL_SIDES, NO_FUSE_LEVEL2 = 1, 2, 4          # DSVG_LOAD_NO_* (include/dsvg.h)
BODIES = ("none", "scalar", "v16", "fused1", "fused2")             # DSVG_UNPACK_*
NONE, SCALAR, V16, FUSED1, FUSED2 = range(5)
BORDERS = (None, "k_extend", "k_extend16")                         # DSVG_BORDER_*
KERNELS = ("k_unpack", "k_extend", "k_extend16", "k_ds2x", "k_luma_sum")       # kernel ids 0..4 (dsvg_host.hpp, DSVG_KERNEL_IDS)
K_UNPACK, K_EXTEND, K_EXTEND16, K_DS2X, K_LUMA_SUM = range(5)

LEVEL_FIELDS = ("w", "h", "border", "tb_only", "ds2x", "ds2x_sides", "ds2x_tail", "src_odd_w", "src_odd_h")
LEVEL_DT = np.dtype([(k, "<i4") for k in LEVEL_FIELDS])
# dsvg_load_plan_out (include/dsvg.h), field for field
PLAN_DT = np.dtype([("levels", "<i4"), ("sides", "<i4"), ("fuse1", "<i4"), ("fuse2", "<i4"), ("sides1", "<i4"), ("sides2", "<i4"), ("body", "<i4", (3,)),
                    ("grid_planes", "<i4"), ("level", LEVEL_DT, (MAX_PYRAMID + 1,)), ("luma_sum", "<i4"), ("luma_sum_dword", "<i4"), ("ring_x16", "<i4"),
                    ("ring_y4", "<i4"), ("chroma_in_place_ok", "<i4"), ("luma_in_place_ok", "<i4"), ("launches", "<i4", (5,)), ("bytes", "<f8", (5,))],
                   align=True)


class Geo:
    """the geometries of a sweep as arrays: luma size, the encoder's block size and its own pyramid depth (dsv_encoder.c:556-613)"""
    def __init__(self, sizes):
        sizes = list(sizes)
        self.w = np.array([s[0] for s in sizes], np.int64)
        self.h = np.array([s[1] for s in sizes], np.int64)
        bd = [block_dims(w, h) for w, h in sizes]
        self.bw = np.array([b[0] for b in bd], np.int64)
        self.bh = np.array([b[1] for b in bd], np.int64)
        self.auto_levels = np.array([pyramid_levels(w, h, b[2], b[3]) for (w, h), b in zip(sizes, bd)], np.int64)


def plane_layout(w, h):
    """(stride, bytes) of one plane in the reference frame layout (frame.c:63-120): 64-px border, stride rounded up to 16"""
    stride = (w + 2 * BORDER + 15) & ~15
    return stride, stride * (h + 2 * BORDER)


def plans(geo, fmt, pyramid=0, with_pyramid=1, src_mod16=0, pitch_mod16=0, switches=0, n=1, n_chroma_in_place=0, n_luma_in_place=0):
    """the plans of every geometry of `geo` at one format and one setting, as an array of PLAN_DT"""
    w, h = geo.w, geo.h
    P = np.zeros(len(w), PLAN_DT)
    hs, vs = (fmt >> 2) & 3, fmt & 3
    cw, ch = rsu(w, hs), rsu(h, vs)
    levels = np.minimum(pyramid, MAX_PYRAMID) + 0 * w if pyramid > 0 else geo.auto_levels
    lw = [rsu(w, l) for l in range(MAX_PYRAMID + 1)]
    lh = [rsu(h, l) for l in range(MAX_PYRAMID + 1)]
    pyr = bool(with_pyramid)
    n_chroma = n - n_chroma_in_place
    no_sides, no_lsides, no_fuse2 = bool(switches & NO_UNPACK_SIDES), bool(switches & NO_LEVEL_SIDES), bool(switches & NO_FUSE_LEVEL2)

    # where things lie: slabs start on 256 bytes, a slot is the frame's planes back to back rounded up to 256, a plane's first pixel
    # 64 rows and 64 bytes into its allocation
    def first_pixel(width, height, planes_before=0):
        stride, _ = plane_layout(width, height)
        return planes_before + stride * BORDER + BORDER, stride

    ystride, ybytes = plane_layout(w, h)
    cstride, cbytes = plane_layout(cw, ch)
    offs0 = [first_pixel(w, h)[0], first_pixel(cw, ch, ybytes)[0], first_pixel(cw, ch, ybytes + cbytes)[0]]
    border16_0 = (ystride % 16 == 0) & (cstride % 16 == 0) & (offs0[0] % 16 == 0) & (offs0[1] % 16 == 0) & (offs0[2] % 16 == 0)
    luma16 = [(first_pixel(lw[l], lh[l])[1] % 16 == 0) & (first_pixel(lw[l], lh[l])[0] % 16 == 0) for l in range(MAX_PYRAMID + 1)]

    # the packed source: frame f at src + f * pitch, its planes back to back
    ysz, csz = w * h, cw * ch
    starts = [0 * w, ysz, ysz + csz]
    every_frame_16 = src_mod16 == 0 and pitch_mod16 == 0          # the address of every frame is a multiple of 16

    def lane16(width, start):
        """k_unpack takes 16-byte lanes for a plane of the call's first frame"""
        return (width % 16 == 0) & ((src_mod16 + start) % 16 == 0)

    # the fused bodies: every frame's luma on 16-byte lanes, rows in pairs (level 1) / fours, both levels exact halvings (levels 1 and 2),
    # and level 2's dword stores aligned
    fuse1 = pyr & (levels >= 1) & (w % 16 == 0) & every_frame_16 & (h % 2 == 0)
    l2_stride, l2_bytes = plane_layout(lw[2], lh[2])
    l2_slot = l2_bytes + 2 * plane_layout(rsu(lw[2], hs), rsu(lh[2], vs))[1]
    l2_dword = (l2_stride % 4 == 0) & (first_pixel(lw[2], lh[2])[0] % 4 == 0) & (((l2_slot + 255) & ~255) % 4 == 0)
    fuse2 = fuse1 & (not no_fuse2) & (levels >= 2) & (h % 4 == 0) & (lw[1] * 2 == w) & (lh[1] * 2 == h) & (lw[2] * 4 == w) & (lh[2] * 4 == h) & l2_dword
    # sides: 16-byte stores into the border beside every row of every plane -- every plane of every frame on 16-byte lanes
    all_lanes16 = every_frame_16 & (w % 16 == 0) & (cw % 16 == 0) & (ysz % 16 == 0) & (csz % 16 == 0)
    sides = all_lanes16 & border16_0 & (not no_sides)

    def level_sides(l):
        return (lw[l] % 16 == 0) & luma16[l]
    sides1 = fuse1 & sides & (not no_lsides) & level_sides(1)
    sides2 = fuse2 & sides & (not no_lsides) & level_sides(2)
    P["levels"], P["sides"], P["fuse1"], P["fuse2"], P["sides1"], P["sides2"] = levels, sides, fuse1, fuse2, sides1, sides2

    # the body k_unpack picks (k_frame.hip: the cascade of `vec && c == 0 && slab1 && slab2 && (h & 3) == 0` ...), handed slab1 / slab2
    # where the host fuses
    vec = lane16(w, starts[0])
    P["body"][:, 0] = np.select([vec & fuse1 & fuse2 & (h % 4 == 0), vec & fuse1 & (h % 2 == 0), vec], [FUSED2, FUSED1, V16], SCALAR)
    for c in (1, 2):
        P["body"][:, c] = np.where(lane16(cw, starts[c]), V16, SCALAR) if n_chroma > 0 else NONE
    P["grid_planes"] = 3 if n_chroma > 0 else 1

    # per-sample figures of the profiler's algorithmic bytes: k_unpack 2 bytes per copied sample, + the levels it writes,
    # less the interior a luma-in-place frame leaves out; a border 8 bytes per dword of the luma border; k_ds2x 5 bytes per mean;
    # k_luma_sum 1 byte per sample
    deep_r = (2 << levels) + 8                                     # k_hme.hip `deep`: a level-0 vector's reach + search + slack
    ring_x16, ring_y4 = (geo.bw + 2 * deep_r + 15) // 16, (geo.bh + 2 * deep_r + 3) // 4
    P["ring_x16"], P["ring_y4"] = ring_x16, ring_y4
    inner = np.maximum(0, w - 32 * ring_x16) * np.maximum(0, h - 8 * ring_y4)
    launches = np.zeros((len(w), 5), np.int64)
    nbytes = np.zeros((len(w), 5), np.float64)
    launches[:, K_UNPACK] = 1
    nbytes[:, K_UNPACK] = 2.0 * (n * ysz + 2.0 * n_chroma * csz) - (n_luma_in_place * inner if n_luma_in_place > 0 else 0) + fuse1 * 0.25 * n * ysz + fuse2 * 0.0625 * n * ysz
    for l in range(MAX_PYRAMID + 1):
        runs = (levels >= l) & (pyr or l == 0)
        fused = fuse1 if l == 1 else fuse2 if l == 2 else np.zeros(len(w), bool)
        if l == 0:
            ls, ds2x = sides, np.zeros(len(w), bool)
        else:
            ls = np.where(fused, sides1 if l == 1 else sides2 if l == 2 else False, (not no_lsides) & level_sides(l)) & runs
            ds2x = runs & ~fused
        e16 = luma16[l] & (lw[l] % 16 == 0) & (border16_0 & (cw % 16 == 0) if l == 0 else True)
        o = P["level"][:, l]
        o["w"], o["h"] = lw[l] * runs, lh[l] * runs
        o["border"] = np.where(runs, np.where(e16, 2, 1), 0)
        o["tb_only"] = ls & runs
        o["ds2x"], o["ds2x_sides"] = ds2x, ds2x & ls
        if l > 0:
            o["ds2x_tail"], o["src_odd_w"], o["src_odd_h"] = ds2x & (lw[l] % 4 != 0), ds2x & (lw[l - 1] % 2 == 1), ds2x & (lh[l - 1] % 2 == 1)
        launches[:, K_DS2X] += ds2x
        nbytes[:, K_DS2X] += ds2x * 5.0 * n * lw[l] * lh[l]
        border_bytes = 8.0 * ((lh[l] + 2 * BORDER) * 32 + 32 * lw[l]) * n
        for k, on in ((K_EXTEND16, runs & e16), (K_EXTEND, runs & ~e16)):
            launches[:, k] += on
            nbytes[:, k] += on * border_bytes
    if pyr:
        tw, th = rsu(w, levels), rsu(h, levels)
        top16 = np.choose(levels, luma16)                          # (its stride and first pixel are multiples of 16, so of 4)
        P["luma_sum"] = 1
        P["luma_sum_dword"] = (tw % 4 == 0) & top16
        launches[:, K_LUMA_SUM] = 1
        nbytes[:, K_LUMA_SUM] = 1.0 * n * tw * th
    P["launches"], P["bytes"] = launches, nbytes

    # in place (dsvg_pipe.hip, dsvg_ctx_create_blk): chroma where the forward transforms' 8-byte patch rows stay inside even planes;
    # luma where k_unpack fuses both levels and the ring leaves an interior of 64 x 64 or more
    cip = (cw % 8 == 0) & (ch % 2 == 0)
    P["chroma_in_place_ok"] = cip
    P["luma_in_place_ok"] = (cip & (levels >= 2) & (w % 16 == 0) & (h % 4 == 0) & (lw[1] * 2 == w) & (lh[1] * 2 == h) & (lw[2] * 4 == w) & (lh[2] * 4 == h) &
                             l2_dword & (32 * ring_x16 + 64 <= w) & (8 * ring_y4 + 64 <= h) & (ring_x16 < 256) & (ring_y4 < 256))
    return P


def as_dict(rec):
    """one record of plans() in the shape of the package's load_plan()"""
    d = {k: int(rec[k]) for k in ("sides", "fuse1", "fuse2", "sides1", "sides2", "grid_planes", "luma_sum", "luma_sum_dword", "ring_x16", "ring_y4",
                                  "chroma_in_place_ok", "luma_in_place_ok")}
    d["body"] = tuple(BODIES[b] for b in rec["body"])
    d["levels"] = []
    for l in range(int(rec["levels"]) + 1):
        lv = {k: int(rec["level"][l][k]) for k in LEVEL_FIELDS if k != "border"}
        lv["border"] = BORDERS[rec["level"][l]["border"]]
        d["levels"].append(lv)
    d["kernels"] = {KERNELS[k]: (int(rec["launches"][k]), float(rec["bytes"][k])) for k in range(5) if rec["launches"][k]}
    return d


def plan(w, h, fmt, **kw):
    """the plan of one geometry (see plans), as a dict"""
    return as_dict(plans(Geo([(w, h)]), fmt, **kw)[0])


# ---- classes ------------------------------------------------------------------------------------------------------------------
# A class is what the plan outputs without the sizes and byte counts.  The levels of a pyramid decide independently of each other, so
# the classes are kept per part, or their product would ask for hundreds of cases that add no branch:
#   "level0": (sides, fuse1, fuse2, sides1, sides2, the three bodies, level 0's border kernel, its tb_only)
#   "upper":  one pyramid level above 0: (border kernel, tb_only, ds2x, ds2x_sides, ds2x_tail, src_odd_w, src_odd_h)
#   "sum":    (luma_sum_dword,)
UPPER_FIELDS = ("border", "tb_only", "ds2x", "ds2x_sides", "ds2x_tail", "src_odd_w", "src_odd_h")


def level0_class(rec):
    return (int(rec["sides"]), int(rec["fuse1"]), int(rec["fuse2"]), int(rec["sides1"]), int(rec["sides2"]), tuple(BODIES[b] for b in rec["body"]),
            BORDERS[rec["level"][0]["border"]], int(rec["level"][0]["tb_only"]))


def upper_classes(rec):
    return [(BORDERS[rec["level"][l]["border"]],) + tuple(int(rec["level"][l][k]) for k in UPPER_FIELDS[1:]) for l in range(1, int(rec["levels"]) + 1)]


def classes(rec):
    """every class a plan belongs to, as (part, tuple)"""
    return [("level0", level0_class(rec))] + [("upper", u) for u in upper_classes(rec)] + [("sum", (int(rec["luma_sum_dword"]),))]


def describe(cls):
    part, t = cls
    if part == "level0":
        s, f1, f2, s1, s2, body, border, tb = t
        return "level0: %s | sides %d%d%d | %s%s" % ("/".join(body), s, s1, s2, border, " tb" if tb else "")
    if part == "upper":
        border, tb, ds, dss, tail, ow, oh = t
        return "upper: %s%s | %s" % (border, " tb" if tb else "", "fused" if not ds else "ds2x%s%s%s%s" % (
            " sides" if dss else "", " tail" if tail else "", " oddw" if ow else "", " oddh" if oh else ""))
    return "sum: %s" % ("dword" if t[0] else "scalar")


SWEEP_MIN, SWEEP_MAX = 32, 300


def sweep_sizes():
    """every even size from 32x32 to 300x300, by area, then width"""
    s = [(w, h) for w in range(SWEEP_MIN, SWEEP_MAX + 1, 2) for h in range(SWEEP_MIN, SWEEP_MAX + 1, 2)]
    return sorted(s, key=lambda g: (g[0] * g[1], g[0], g[1]))


@functools.lru_cache(maxsize=None)
def sweep_geo():
    return Geo(sweep_sizes())


@functools.lru_cache(maxsize=None)
def sweep(pyramid=0):
    """{class: (w, h, fmt) of the smallest geometry of the sweep that has it} at the default switches, an aligned source, the given
    pyramid depth (0: the encoder's own); ties by area go to the earlier format of FORMATS, then the narrower picture"""
    geo = sweep_geo()
    best = {}

    def first_of_each(P, columns, keep):
        """indices (among the records where `keep`) of the first record of every distinct row of `columns`: the sizes come by area"""
        rows = np.nonzero(keep)[0]
        _, first = np.unique(np.column_stack([c[rows] for c in columns]), axis=0, return_index=True)
        return rows[first]

    for fi, fmt in enumerate(FORMATS.values()):
        P = plans(geo, fmt, pyramid=pyramid)
        every = np.ones(len(P), bool)
        cand = set(first_of_each(P, [P[k] for k in ("sides", "fuse1", "fuse2", "sides1", "sides2")] + [P["body"][:, c] for c in range(3)] +
                                 [P["level"][:, 0]["border"], P["level"][:, 0]["tb_only"]], every))
        cand |= set(first_of_each(P, [P["luma_sum_dword"]], every))
        for l in range(1, MAX_PYRAMID + 1):
            if (P["levels"] >= l).any():
                cand |= set(first_of_each(P, [P["level"][:, l][k] for k in UPPER_FIELDS], P["levels"] >= l))
        for i in sorted(cand):
            key = (int(geo.w[i] * geo.h[i]), fi, int(geo.w[i]))
            for c in classes(P[i]):
                if c not in best or key < best[c][0]:
                    best[c] = (key, (int(geo.w[i]), int(geo.h[i]), fmt))
    return {c: g for c, (k, g) in best.items()}
