"""The product's plan for the inverse transform of one picture, restated from the host code (host arithmetic only).

Given a geometry (w, h, fmt) this says which kernels `launch_inv_sbt` / `launch_inv54_all` (csrc/k_sbt.hip) launch for the
reconstruction of an encoder picture, with which sub-branch, and how many launches and algorithmic bytes (the `PB(...)`
figures the per-kernel profiler adds up) each kernel gets per picture.  It restates the product's planning, not the
reference: what is right is decided by the oracle; this module only says which code a geometry reaches, so that the
tests can name the branch a case is there for and check on the GPU that it was taken.

Every rule cites the line it restates.  Line numbers refer to csrc/k_sbt.hip unless another file is named.
"""
import collections
import re

IT_TX, IT_TY = 16, 8          # level-3 cells per tile of the inverse kernels (k_sbt.hip:2144-2145)
BT_CX, BT_CY = 60, 32         # level-1 cells per tile of k_inv_b4t (k_sbt.hip:3110-3113)
BORDER = 64                   # DSVG_BORDER: the reference frame's border (dsvg_common.hip:95)
FORMATS = {"444": 0x0, "422": 0x4, "420": 0x5, "411": 0x8}

# kernel names exactly as DSVG_KERNEL_IDS spells them (dsvg_host.hpp:56-73)
K54_ALL = "k_inv_tile54_all"
K54_F, K54 = "void k_inv_haar_tile<true, 2, false>", "void k_inv_haar_tile<false, 2, false>"
KTAIL = "k_inv_tail"
KP_TILE_F, KP_TILE = "void k_inv_p_tile<true>", "void k_inv_p_tile<false>"
KPIX_SYM_F, KPIX_SYM = "void k_inv_haar_tile<true, 0, true>", "void k_inv_haar_tile<false, 0, true>"
KPIX_F, KPIX = "void k_inv_haar_tile<true, 0, false>", "void k_inv_haar_tile<false, 0, false>"
KS1_F, KS1 = "void k_inv_haar_tile<true, 1, false>", "void k_inv_haar_tile<false, 1, false>"
KS1_SYM_F, KS1_SYM = "void k_inv_haar_tile<true, 1, true>", "void k_inv_haar_tile<false, 1, true>"
KB4T, KB4T_SYM = "void k_inv_b4t<false>", "void k_inv_b4t<true>"
KPATCH_C = "k_inv_patch_c"
re_inverse = re.compile(r"(void )?k_inv_")        # the names of the inverse kernels

Geo = collections.namedtuple("Geo", "W H pw ph pstride w3 h3 w5 h5 l1a")


def rsu(x, s):
    return (x + (1 << s) - 1) >> s


def plane_geos(w, h, fmt):
    """SbtGeo of the three planes as dsvg_ctx_create_blk builds them (dsvg_pipe.hip:495-506)"""
    hs, vs = (fmt >> 2) & 3, fmt & 3                                       # fmt_hs / fmt_vs (dsvg_host.hpp:26-27)
    cw, ch = rsu(w, hs), rsu(h, vs)                                        # make_frame_layout (dsvg_common.hip:98)
    out = []
    for c in range(3):
        pw, ph = (cw, ch) if c else (w, h)
        pstride = (pw + 2 * BORDER + 15) & ~15                             # dsvg_common.hip:103
        W, H = ((cw + 1) & ~1, (ch + 1) & ~1) if c else (w, h)             # make_coef_layout: chroma rounded up to even (dsvg_common.hip:142-145)
        w3, h3, w2, h2, w1, h1 = rsu(W, 3), rsu(H, 3), rsu(W, 2), rsu(H, 2), rsu(W, 1), rsu(H, 1)
        # l1a (dsvg_pipe.hip:505): scan regions 7..9 of make_hz_plane (dsvg_common.hip:171-196) -- the level-1 bands -- start and
        # run in multiples of 4 cells.  Region 7 starts behind LL3 and the six level-3 / level-2 detail bands.
        base7 = 4 * w3 * h3 + 3 * w2 * h2
        l1a = ((w1 | base7 | (base7 + w1 * h1) | (base7 + 2 * w1 * h1)) & 3) == 0
        out.append(Geo(W, H, pw, ph, pstride, w3, h3, rsu(W, 5), rsu(H, 5), l1a))
    return out


def fuses_border(G):
    """inv_sbt_fuses_border (k_sbt.hip:3432-3447) for the encoder's P chroma (insym_c = patch_kernel_c = 1), without its A/B
    switches: (fb, hr, vr)"""
    g, gy = G[1], G[0]
    for q in (G[1], G[2]):
        if q.pw != g.pw or q.ph != g.ph or q.w3 != g.w3 or q.h3 != g.h3 or q.pw & 15 or q.pstride & 15:     # :3439
            return False, 0, 0
        fullc, fullr = q.pw // 8, q.ph // 8                                                                # :3440
        part4 = fullr == q.h3 - 1 and fullr >= 1 and (q.ph & 7) == 4 and (q.H & 7) == 4                   # :3441
        if fullc < q.w3 or not (fullr >= q.h3 or part4):                                                   # :3442
            return False, 0, 0
    if g.pw < 16 or g.ph < 8 or gy.pw % g.pw or gy.ph % g.ph or gy.pstride & 15 or gy.pw & 15:           # :3444
        return False, 0, 0
    hr, vr = gy.pw // g.pw, gy.ph // g.ph                                                                  # :3445
    return (hr in (1, 2, 4) and vr in (1, 2)), hr, vr                                                      # :3446


def _add(k, name, nbytes):
    n, b = k.get(name, (0, 0.0))
    k[name] = (n + 1, b + nbytes)


def luma_p(g, k):
    """launch_inv_sbt, luma of a P picture from the symbol planes with the patch kernel (insym = patch_kernel = 1, filt):
    k_sbt.hip:3498-3529.  Returns the branch."""
    tgx, tgy = -(-g.w3 // IT_TX), -(-g.h3 // IT_TY)                                                         # tg (:3469)
    smp = float(g.W * g.H)                                                                                 # (:3455, nz = 1)
    fx = (g.w3 - IT_TX - 2) // IT_TX + 1 if g.l1a and g.w3 >= IT_TX + 2 else 0                              # :3502
    fy = (g.h3 - IT_TY - 2) // IT_TY + 1 if g.l1a and g.h3 >= IT_TY + 2 else 0                              # :3503
    if fx > 0 and fy > 0:                                                                                  # :3505
        er = fx == tgx - 1 and g.w3 == tgx * IT_TX and (g.W & 7) == 0                                       # :3507
        eb = fy == tgy - 1 and (g.H & 7) == 0                                                               # :3509
        fxg, fyg = fx + er, fy + eb                                                                         # :3510
        fsmp = 64.0 * min(fxg * IT_TX, g.w3) * min(fyg * IT_TY, g.h3)                                       # :3511
        _add(k, KP_TILE_F, fsmp * 2.5)                                                                      # :3512-3516
        nrest = (tgx - fxg) * tgy + fxg * (tgy - fyg)                                                       # :3517
        if nrest > 0:
            _add(k, KPIX_SYM_F, (smp - fsmp) * 2.5)                                                         # :3518-3523
        return dict(kind="fast", fx=fx, fy=fy, er=er, eb=eb, fxg=fxg, fyg=fyg, nrest=nrest, l1a=g.l1a,
                    strip_cols=tgx - fxg, strip_rows=tgy - fyg)
    _add(k, KPIX_SYM_F, smp * 2.5)                                                                          # :3526-3529
    return dict(kind="general", l1a=g.l1a, fx=fx, fy=fy)


def chroma_p(G, k):
    """launch_inv_sbt, both chroma planes of a P picture in one launch (c0 = 1, npl = 2, insym = patch_kernel = 1, no filter):
    k_sbt.hip:3473-3497.  Returns the branch."""
    g = G[1]
    nz = 2
    tgx, tgy = -(-g.w3 // IT_TX), -(-g.h3 // IT_TY)
    smp = float(g.W * g.H * nz)
    fullc, fullr = g.pw // 8, g.ph // 8                                                                     # :3476
    part4 = fullr == g.h3 - 1 and fullr >= 1                                                                # :3480
    part4 = part4 and all(q.ph == g.ph and (q.ph & 7) == 4 and (q.H & 7) == 4 and q.h3 == g.h3 for q in G[1:])   # :3481
    tcx = tgx if fullc >= g.w3 else fullc // IT_TX                                                          # :3482
    tcy = tgy if (fullr >= g.h3 or part4) else fullr // IT_TY
    imax = g.w3 if tcx >= tgx else tcx * IT_TX                                                              # :3483
    jmax = g.h3 if tcy >= tgy else tcy * IT_TY
    if imax > 0 and jmax > 0:                                                                               # :3484-3490
        _add(k, KPATCH_C, 64.0 * imax * jmax * nz * 2.0)
    nrest = 0
    if tcx < tgx or tcy < tgy:                                                                              # :3491-3497
        _add(k, KPIX_SYM, (smp - 64.0 * imax * jmax * nz) * 2.5)
        nrest = (tgx - tcx) * tgy + tcx * (tgy - tcy)                                                       # :3494
    fb, hr, vr = fuses_border(G)                                                                           # :3452 (and dsvg_pipe.hip:1231)
    return dict(imax=imax, jmax=jmax, part4=part4, tcx=tcx, tcy=tcy, right_strip=tcx < tgx, bottom_strip=tcy < tgy,
                nrest=nrest, fb=fb, hr=hr if fb else 0, vr=vr if fb else 0)


def intra(G, k):
    """launch_inv_sbt of an I picture from the symbol planes (insym = 1), luma then chroma: k_sbt.hip:3536-3551"""
    for c0, npl in ((0, 1), (1, 2)):
        g = G[c0]
        smp = float(g.W * g.H * npl)
        _add(k, KS1_SYM_F if c0 == 0 else KS1_SYM, smp * 1.4)                                               # :3537-3540
        _add(k, KB4T_SYM, smp * 3.5)                                                                        # :3547-3548


class Plan:
    """the encoder's inverse transform of one picture per frame step of one coding stream (a call of one frame)

    luma, chroma   -- the P picture's branches (dicts, see luma_p / chroma_p)
    p_kernels      -- {kernel name: (launches, algorithmic bytes)} of the inverse kernels of one P picture
    i_kernels      -- the same of one I picture
    cls            -- the dispatch class: (luma branch, chroma branch, fused-border ratio)
    """

    def __init__(self, w, h, fmt):
        self.w, self.h, self.fmt = w, h, fmt
        self.geos = G = plane_geos(w, h, fmt)
        s3 = float(sum(g.w3 * g.h3 for g in G))
        # the encoder (dsvg_pipe.hip:1524,1536): k_tail_q did the inverse tail (tail_done), levels 5..4 of all planes in one
        # launch (enqueue_recon, dsvg_pipe.hip:1219-1221; launch_inv54_all :3416-3427), lazy borders on
        self.p_kernels, self.i_kernels = {}, {}
        for k in (self.p_kernels, self.i_kernels):
            _add(k, K54_ALL, s3 * 8.0)
        intra(G, self.i_kernels)
        # P pictures: symY = symC = patch kernel = 1 (enqueue_recon(.., 7, ..) dsvg_pipe.hip:1228,1232-1233)
        self.luma = luma_p(G[0], self.p_kernels)
        self.chroma = chroma_p(G, self.p_kernels)
        self.cls = (luma_class(self.luma), chroma_class(self.chroma), (self.chroma["hr"], self.chroma["vr"]))

    def __repr__(self):
        return "Plan(%dx%d fmt=%#x: %s)" % (self.w, self.h, self.fmt, describe(self.cls))


def luma_class(b):
    if b["kind"] == "general":
        return ("general", "l1a" if b["l1a"] else "no-l1a")
    return ("fast", "er" if b["er"] else "-", "eb" if b["eb"] else "-", "strips" if b["nrest"] else "-")


def chroma_class(b):
    if b["imax"] == 0 or b["jmax"] == 0:
        # no whole patch outside the edge tiles: the L-shaped strip launch is every tile of the planes (tcx or tcy = 0), whatever
        # part4 and the strips say
        return ("no-patch",)
    return ("patch", "part4" if b["part4"] else "-", "right" if b["right_strip"] else "-", "bottom" if b["bottom_strip"] else "-")


def describe(cls):
    l, c, (hr, vr) = cls
    return "luma %s | chroma %s | %s" % ("/".join(map(str, l)), "/".join(c), ("fb %dx%d" % (hr, vr)) if hr else "no fb")


def plan(w, h, fmt):
    return Plan(w, h, fmt)


def scan_overlap(w, h, fmt):
    """the HZCC scan regions of luma or chroma overlap (dsvg_pipe.hip:528-532, dec_ov): a shared cell can be quantised to 0 in the
    encoder's second pass while the decoder keeps the first symbol -- the reference's decoder then drifts from its encoder's
    reconstruction (tests/test_gpu_stream.py, _decode_and_compare)"""
    for g in plane_geos(w, h, fmt)[:2]:
        sw, sh = [rsu(g.W, 3 - l) for l in range(3)], [rsu(g.H, 3 - l) for l in range(3)]
        if 2 * sw[0] > sw[1] or 2 * sh[0] > sh[1] or 2 * sw[1] > sw[2] or 2 * sh[1] > sh[2]:
            return True
    return False


def coded_geometry(w, h):
    """what dsvg_ctx_create accepts: luma at least 32x32 (dsvg_pipe.hip:475), even (:512)"""
    return w >= 32 and h >= 32 and not (w | h) & 1


def sweep(wmax=1300, hmax=760, keep=3):
    """{class: the `keep` smallest geometries (w, h, fmt) of the class by area} over every even geometry the encoder accepts up to
    wmax x hmax, in all four formats"""
    seen = {}
    for fmt in FORMATS.values():
        for h in range(32, hmax + 1, 2):
            for w in range(32, wmax + 1, 2):
                c = Plan(w, h, fmt).cls
                k = seen.setdefault(c, [])
                if len(k) < keep or w * h < k[-1][0]:
                    k.append((w * h, w, h, fmt))
                    k.sort()
                    del k[keep:]
    return {c: [g[1:] for g in k] for c, k in seen.items()}


# the op-level twin (dsvg_op_inv_sbt, dsvg_ops.hip:157) calls launch_inv_sbt(.., isP) with the defaults insym = 0, with_tail = 1
# (dsvg_kernels.hpp:46-48): the inverse tail, levels 5..4 per plane, then the int32-coefficient kernels (k_sbt.hip:3457-3468,
# 3530-3535, 3536-3551), luma (filt) and chroma alike; tests/test_gpu_ops.py::test_fwd_inv_sbt drives it with c = 0 and 1
TWIN_KERNELS = {KTAIL, K54_F, K54, KPIX_F, KPIX, KS1_F, KS1, KB4T}

# inverse kernel ids no matrix case reaches, and why
UNREACHABLE = {
    KP_TILE: "k_inv_p_tile<false> needs insym with patch_kernel and no filter, but every unfiltered plane (chroma) with "
             "patch_kernel takes k_inv_patch_c first (k_sbt.hip:3473 before :3498, :3515)",
}
