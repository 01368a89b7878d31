"""The product's plan for the analysis and forward half of one encoder picture, restated from the host code (host arithmetic only).

Given a geometry (w, h, fmt) this says which block size the encoder takes, whether motion compensation is fused into the forward
transform, which branch `fwd_sbt_plan` (csrc/k_sbt.hip) takes for the general kernel of luma and of the chroma pair, what
`hme_plan` (csrc/k_hme.hip) launches per pyramid level, and how many launches and algorithmic bytes (the steps' `bytes`, which
the executors hand to the per-kernel profiler's brackets) each forward and motion-search kernel gets per picture.  It restates the
product's planning, not the reference: what is right is decided by the oracle; this module only says which code a geometry
reaches, so that the tests can name the branch a case is there for and check that it was taken -- on the GPU against the profiler
and dsvg_dispatch_last, on the CPU against the plans the launchers execute (dsvg_dispatch_plan, dsvg_fwd_plan, dsvg_hme_plan)
over the matrix and a sample of the sweep.

Every rule cites the line it restates.  Line numbers refer to csrc/k_sbt.hip unless another file is named.
"""
import functools

from inv_plan import BORDER, FORMATS, rsu

# kernel names exactly as DSVG_KERNEL_IDS spells them (dsvg_host.hpp:56-73)
K_MC = "k_mc"
K_FAST_Y, K_FAST_C = "void k_fwd_mc_fast<0>", "void k_fwd_mc_fast<1>"
K_PIX_Y, K_PIX_C = "void k_fwd_mc_pix<0>", "void k_fwd_mc_pix<1>"
K_HAAR_PIX_Q = "void k_fwd_haar_pix<true>"
K_B4T_Q, K_MID2_Q = "void k_fwd_b4t<true>", "void k_fwd_haar_mid<2, true>"
K_MID4, K_TAIL_Q = "void k_fwd_haar_mid<4, false>", "k_tail_q"
K_HME_UP, K_HME_L0, K_HME_DETAIL, K_HME_CSUM = "void k_hme_level<false>", "void k_hme_level<true>", "k_hme_detail", "k_hme_csum"
FORWARD_KERNELS = [K_MC, K_FAST_Y, K_FAST_C, K_PIX_Y, K_PIX_C, K_HAAR_PIX_Q, K_B4T_Q, K_MID2_Q, K_MID4, K_TAIL_Q,
                   "void k_fwd_haar_pix<false>", "void k_fwd_b4t<false>", "void k_fwd_haar_mid<2, false>", "k_fwd_tail"]
K_HZ_SCAN = "k_hz_scan"
SEARCH_KERNELS = [K_HME_UP, K_HME_L0, K_HME_DETAIL, K_HME_CSUM]

# DSVG_FWD_* (include/dsvg.h): what dsvg_dispatch reports per plane group
WHOLE, TOP, BOTTOM, LEFT, RIGHT, ROW1, COL1 = 1, 2, 4, 8, 16, 32, 64
MAX_PYRAMID = 5               # DSVG_MAX_PYRAMID (include/dsvg.h:43)


def block_dims(w, h):
    """block_geometry (dsvg_common.hip:202-212): (blk_w, blk_h, nbh, nbv)"""
    def s4(d):
        s = 64 if d > 1280 else 48 if d > 1024 else 32 if d > 704 else 24 if d > 352 else 16
        return min(max(s & ~7, 16), 64)
    bw, bh = s4(w), s4(h)
    return bw, bh, (w + bw - 1) // bw, (h + bh - 1) // bh


def lb2(n):
    """dsvg_lb2u (dsvg_dev.hpp:176-182): ceil(log2 n)"""
    return (n - 1).bit_length()


def pyramid_levels(w, h, nbh, nbv):
    """auto_pyramid_levels (dsvg_common.hip:214-220)"""
    lv = lb2(min(w, h))
    while (1 << lv) > max(nbh, nbv):
        lv -= 1
    return min(max(lv, 3), MAX_PYRAMID)


def plane_dims(w, h, fmt):
    """[(pixel w, pixel h, coefficient W, coefficient H)] of the three planes: make_frame_layout (dsvg_common.hip:96-102) and
    make_coef_layout (dsvg_common.hip:142-146: chroma rounded up to even)"""
    hs, vs = (fmt >> 2) & 3, fmt & 3
    cw, ch = rsu(w, hs), rsu(h, vs)
    return [(w, h, w, h)] + [(cw, ch, (cw + 1) & ~1, (ch + 1) & ~1)] * 2


def fusable(w, h, fmt):
    """mc_fusable (k_sbt.hip:3266-3269; dsvg_pipe.hip: c->mc_fused)"""
    bw, bh, _, _ = block_dims(w, h)
    hs, vs = (fmt >> 2) & 3, fmt & 3
    return (bw >> hs) % 8 == 0 and (bh >> vs) % 8 == 0 and bw % 8 == 0 and bh % 8 == 0


@functools.lru_cache(maxsize=None)
def x_facts(W, pw, nbh):
    """the horizontal half of fwd_general_mask for one plane (k_sbt.hip:3298-3316): (left, right, whole, one column of thread
    blocks)"""
    sw0, sw1, sw2 = rsu(W, 3), rsu(W, 2), rsu(W, 1)
    left = 2 * sw0 > sw1 or 2 * sw1 > sw2                                                    # :3305
    right = (pw & 7) != 0                                                                    # :3307 (mc.w[c]: the pixel plane)
    d1, d2 = (nbh << 14) // sw2, (nbh << 14) // sw1                                          # :3309
    whole = any(((4 * i * d1) >> 14) != (((4 * i + 3) * d1) >> 14) or ((2 * i * d2) >> 14) != (((2 * i + 1) * d2) >> 14)
                for i in range(sw0))                                                         # :3310-3311
    return left, right, whole, (sw0 + 63) // 64 == 1                                         # grid3 (:3247), :3313


@functools.lru_cache(maxsize=None)
def y_facts(H, ph):
    """the vertical half: (top, bottom, one row of thread blocks)"""
    sh0, sh1, sh2 = rsu(H, 3), rsu(H, 2), rsu(H, 1)
    top = 2 * sh0 > sh1 or 2 * sh1 > sh2                                                     # :3306
    bottom = (ph & 7) != 0                                                                   # :3308 (gc.ph)
    return top, bottom, (sh0 + 3) // 4 == 1                                                  # grid3: 4 patch rows per thread block


def general_mask(w, h, fmt, group):
    """fwd_general_mask (k_sbt.hip:3298-3316) of plane group 0 (luma) / 1 (the chroma pair, whose planes are alike), as the
    encoder calls it (dsvg_pipe.hip: launch_fwd_sbt(.., &c->MG, mv0, gw); with FWD_FAST_INTRA = 1 (k_sbt.hip:852) `gw` does not
    enter the decision)"""
    pw, ph, W, H = plane_dims(w, h, fmt)[group]
    nbh = block_dims(w, h)[2]
    left, right, whole, col1 = x_facts(W, pw, nbh)
    top, bottom, row1 = y_facts(H, ph)
    return (WHOLE * whole | TOP * top | BOTTOM * bottom | LEFT * left | RIGHT * right | ROW1 * row1 | COL1 * col1)


def general_branch(mask):
    """the branch fwd_sbt_plan takes for the general kernel (k_sbt.hip:3352-3363): (name, launches).  Names: 'whole', or
    '<rows>|<cols>' with rows in - / row1 (a one-row grid: fy == 1) / T+B / T / B and cols in - / col1 / L+R / L / R"""
    if mask & WHOLE:
        return "whole", 1                                                                    # :3352
    t, b, l, r = mask & TOP, mask & BOTTOM, mask & LEFT, mask & RIGHT
    rows = "row1" if (t or b) and mask & ROW1 else "T+B" if t and b else "T" if t else "B" if b else "-"     # :3355-3358
    cols = "col1" if (l or r) and mask & COL1 else "L+R" if l and r else "L" if l else "R" if r else "-"     # :3359-3362
    return rows + "|" + cols, (rows != "-") + (cols != "-")


def general_strips(mask, fx, fy):
    """the general kernel's launches over the fx x fy grid of thread blocks of a plane group (grid3 of its first plane, :3325), the
    strip ladder of fwd_sbt_plan (k_sbt.hip:3352-3363): [(grid x, grid y, bxofs, byofs, bxstep, bystep)] -- thread block (x, y) of a
    launch works on block (bxofs + x * bxstep, byofs + y * bystep) of the full grid (k_fwd_mc_pix)"""
    if mask & WHOLE:
        return [(fx, fy, 0, 0, 1, 1)]                                                        # :3352
    t, b, l, r = mask & TOP, mask & BOTTOM, mask & LEFT, mask & RIGHT
    out = []
    if (t or b) and fy == 1:
        out.append((fx, 1, 0, 0, 1, 1))                                                      # :3355
    elif t and b:
        out.append((fx, 2, 0, 0, 1, fy - 1))                                                 # :3356: block rows 0 and fy - 1
    elif t:
        out.append((fx, 1, 0, 0, 1, 1))                                                      # :3357
    elif b:
        out.append((fx, 1, 0, fy - 1, 1, 1))                                                 # :3358
    if (l or r) and fx == 1:
        out.append((1, fy, 0, 0, 1, 1))                                                      # :3359
    elif l and r:
        out.append((2, fy, 0, 0, fx - 1, 1))                                                 # :3360: block columns 0 and fx - 1
    elif l:
        out.append((1, fy, 0, 0, 1, 1))                                                      # :3361
    elif r:
        out.append((1, fy, fx - 1, 0, 1, 1))                                                 # :3362
    return out


def hme_level(w, h, level):
    """hme_level_plan (k_hme.hip:1476-1491) for an encoder context: (nkbf, fullx, fully, parts mask, nrest)"""
    bw, bh, nbh, nbv = block_dims(w, h)
    step = 1 << level
    nvx, nvy = (nbh + step - 1) // step, (nbv + step - 1) // step                            # k_hme.hip:1479
    fw, fh = rsu(w, level), rsu(h, level)                                                    # c->L[l] (dsvg_pipe.hip: make_frame_layout(.., rsu(width, l), ..))
    stride = (fw + 2 * BORDER + 15) & ~15                                                    # dsvg_common.hip:103
    nkbf = bh // 4 if bw == 64 and bh in (64, 48, 32) and stride & 3 == 0 else 0             # k_hme.hip:1483
    fullx, fully = (min(nvx, fw // 64), min(nvy, fh // bh)) if nkbf else (0, 0)              # k_hme.hip:1485
    nfull = fullx * fully
    nrest = nvx * nvy - nfull                                                                # k_hme.hip:1486
    if nfull > 0 and level > 0:
        parts = 1 << 3                                                                       # k_hme.hip:1487
    elif nfull > 0:
        parts = 1 << 1 | (1 << 2 if nrest > 0 else 0)                                        # k_hme.hip:1488
    else:
        parts = 1 << 0                                                                       # k_hme.hip:1489
    return nkbf, fullx, fully, parts, nrest


def hme_csum(w, h, fmt):
    """hme_csum_plan (k_hme.hip:1468-1474; the kernel's own test k_hme.hip:1410): 0 not launched, 1 launched, 2 launched and
    returns at once"""
    bw, bh, nbh, nbv = block_dims(w, h)
    fullb = bw == 64 and bh in (64, 48, 32)                                                  # (the stride is a multiple of 16)
    fullx, fully = (min(nbh, w // 64), min(nbv, h // bh)) if fullb else (0, 0)
    if not (fullx > 0 and fully > 0):
        return 0
    return 2 if (bw >> ((fmt >> 2) & 3)) & 15 or fullx > 64 else 1


def hme_class(w, h, fmt):
    """the motion search's dispatch class: (NKBF, level 0's PARTs, the kinds of upper levels, k_hme_csum).  Upper levels: '0' the
    generic body alone (PART 0), '3' one PART 3 launch with full and partial blocks, '3f' one PART 3 launch of full blocks only"""
    bw, bh, nbh, nbv = block_dims(w, h)
    levels = pyramid_levels(w, h, nbh, nbv)
    nkbf, _, _, parts, _ = hme_level(w, h, 0)
    l0 = "+".join(str(p) for p in range(4) if parts >> p & 1)
    up = set()
    for l in range(1, levels + 1):
        _, _, _, p, nrest = hme_level(w, h, l)
        up.add("0" if p == 1 else "3" if nrest else "3f")
    return nkbf, l0, "/".join(sorted(up)), ("none", "table", "early-out")[hme_csum(w, h, fmt)]


def tail_threads(njobs):
    """the variants of k_tail_q (fwd_step_plan, k_sbt.hip:3387) and k_hz_scan (k_hzcc.hip:1764-1765) for njobs jobs of three planes"""
    return 1024 if 3 * njobs <= 96 else 256


def _add(k, name, nbytes, n=1):
    a, b = k.get(name, (0, 0.0))
    k[name] = (a + n, b + nbytes)


class Plan:
    """the analysis and forward half of one picture per frame step of one stream (a call of one frame)

    blk            -- (blk_w, blk_h, nbh, nbv)
    fusable        -- motion compensation inside the forward transform
    masks, luma, chroma -- the general kernel's DSVG_FWD_* masks and branches of a P picture (None where not fusable)
    hme            -- per level 0..levels: (nkbf, fullx, fully, parts mask)
    csum           -- hme_csum
    i_kernels      -- {kernel name: (launches, algorithmic bytes)} of the forward kernels of one I picture (no motion search)
    p_kernels(intra) -- the same of one P picture, motion search included; intra: the picture has intra blocks
    """

    def __init__(self, w, h, fmt):
        self.w, self.h, self.fmt = w, h, fmt
        self.blk = block_dims(w, h)
        self.fusable = fusable(w, h, fmt)
        self.levels = pyramid_levels(w, h, self.blk[2], self.blk[3])
        self.dims = D = plane_dims(w, h, fmt)
        self.masks = tuple(general_mask(w, h, fmt, g) for g in (0, 1)) if self.fusable else (-1, -1)
        self.luma, self.chroma = (general_branch(m)[0] if self.fusable else None for m in self.masks)
        self.hme = tuple(hme_level(w, h, l)[:4] for l in range(self.levels + 1))
        self.csum = hme_csum(w, h, fmt)
        self.hme_cls = hme_class(w, h, fmt)
        # coefficient samples of luma and of the chroma pair (smp, :3324), level-3 and level-5 cells of all planes
        self.smp = (float(D[0][2] * D[0][3]), float(D[1][2] * D[1][3] * 2))
        s3 = float(sum(rsu(d[2], 3) * rsu(d[3], 3) for d in D))
        s5 = float(sum(rsu(d[2], 5) * rsu(d[3], 5) for d in D))
        # every picture: levels 4..5 of all planes in one launch (mid4_step :3273-3284), then the tail with the LL quantiser
        # (tail_step :3286-3295): fwd_step_plan :3379-3389, from enqueue_group (dsvg_pipe.hip)
        self.common = {}
        _add(self.common, K_MID4, s3 * 8.0)
        _add(self.common, K_TAIL_Q, s5 * 8.0)
        # I pictures, luma then the chroma pair: k_fwd_b4t<true> + k_fwd_haar_mid<2, true> (:3367-3369, quantised)
        self.i_kernels = dict(self.common)
        for smp in self.smp:
            _add(self.i_kernels, K_B4T_Q, smp * 3.5)
            _add(self.i_kernels, K_MID2_Q, smp * 1.4)

    def p_kernels(self, intra):
        k = dict(self.common)
        if self.fusable:
            # :3334-3363: the lean kernel over the whole grid, the general kernel per branch; k_mc serves the intra blocks by list
            # (dsvg_pipe.hip: `if (icnt[..]) launch_mc(.., list)`, k_bmc.hip:386-391)
            for g, (fast, pix) in enumerate(((K_FAST_Y, K_PIX_Y), (K_FAST_C, K_PIX_C))):
                _add(k, fast, self.smp[g] * 3.0)
                n = general_branch(self.masks[g])[1]
                if n:
                    _add(k, pix, 0.0, n)
            if intra:
                _add(k, K_MC, 0.0)
        else:
            # k_mc over every block (k_bmc.hip:393: pixel planes, 4 B/sample), then k_fwd_haar_pix<true> (:3365)
            _add(k, K_MC, float(sum(d[0] * d[1] for d in self.dims)) * 4.0)
            for smp in self.smp:
                _add(k, K_HAAR_PIX_Q, smp * 3.0)
        # the motion search of the picture's pair (hme_plan k_hme.hip:1495-1537, npairs = 1; the chroma table is on)
        cpx = float(self.dims[1][0] * self.dims[1][1] + self.dims[2][0] * self.dims[2][1])
        if self.csum:
            _add(k, K_HME_CSUM, cpx)                                                         # k_hme.hip:1507
        for l in range(self.levels, 0, -1):
            _add(k, K_HME_UP, 2.0 * rsu(self.w, l) * rsu(self.h, l))                         # k_hme.hip:1514,1527: one bracket per level
        _add(k, K_HME_L0, 2.0 * self.w * self.h)                                             # (level 0's PART 1 + PART 2 share one bracket)
        _add(k, K_HME_DETAIL, 0.0)                                                           # k_hme.hip:1535
        return k

    def dispatch(self):
        """what dsvg_dispatch_plan / dsvg_dispatch_last report (the package's Dispatch.as_dict)"""
        return {"blk": self.blk[:2], "fusable": int(self.fusable), "fwd": self.masks, "csum": self.csum, "hme": self.hme, "threads": (-1, -1)}

    def axes(self):
        """the values of the independent axes this geometry has: {axis: value}"""
        a = {"fusable": (self.fusable, self.fmt), "hme": self.hme_cls}
        if self.fusable:
            a["luma"], a["chroma"] = self.luma, self.chroma
        return a

    def __repr__(self):
        return "Plan(%dx%d fmt=%#x: %s)" % (self.w, self.h, self.fmt, self.axes())


def plan(w, h, fmt):
    return Plan(w, h, fmt)


def coded_geometry(w, h):
    """what dsvg_ctx_create accepts: luma at least 32x32 (dsvg_pipe.hip:477), even (:490)"""
    return w >= 32 and h >= 32 and not (w | h) & 1


# The sweep: every even geometry up to SWEEP_W x SWEEP_H (blocks 64 wide need w > 1280; NKBF 16 needs h > 1280, and a picture
# tiled by full 64x64 blocks 1344x1344), and a strip of the widths whose 65 or more full block columns make k_hme_csum return at
# once, at the smallest heights with 64-wide blocks.
SWEEP_W, SWEEP_H = 1400, 1400
WIDE = (range(4160, 4226, 2), range(706, 738, 2))


def sweep_domain():
    for h in range(32, SWEEP_H + 1, 2):
        for w in range(32, SWEEP_W + 1, 2):
            yield w, h
    for h in WIDE[1]:
        for w in WIDE[0]:
            yield w, h


def sweep(keep=3):
    """{(axis, value): the `keep` smallest geometries (w, h, fmt) by area} over the sweep's domain in all four formats; the
    same rules as Plan.axes, asked once per size where the format does not enter"""
    seen = {}

    def note(key, w, h, fmt):
        k = seen.setdefault(key, [])
        if len(k) < keep or (w * h, w, h, fmt) < k[-1]:
            k.append((w * h, w, h, fmt))
            k.sort()
            del k[keep:]

    for w, h in sweep_domain():
        nbh = block_dims(w, h)[2]
        hme = hme_class(w, h, 0)[:3]
        l, r, whole, col1 = x_facts(w, w, nbh)
        t, b, row1 = y_facts(h, h)
        luma = general_branch(WHOLE * whole | TOP * t | BOTTOM * b | LEFT * l | RIGHT * r | ROW1 * row1 | COL1 * col1)[0]
        for fmt in FORMATS.values():
            f = fusable(w, h, fmt)
            note(("fusable", (f, fmt)), w, h, fmt)
            note(("hme", hme + (("none", "table", "early-out")[hme_csum(w, h, fmt)],)), w, h, fmt)
            if f:
                note(("luma", luma), w, h, fmt)
                note(("chroma", general_branch(general_mask(w, h, fmt, 1))[0]), w, h, fmt)
    return {k: [g[1:] for g in v] for k, v in seen.items()}
