"""The product's plan for the inverse transform of one picture, restated from the host code (host arithmetic only).

Given a geometry (w, h, fmt) this says which kernels `launch_inv_sbt` / `launch_inv54_all` (csrc/k_sbt.hip) launch for the
reconstruction of an encoder picture, with which sub-branch, and how many launches and algorithmic bytes (the `PB(...)`
figures the per-kernel profiler adds up) each kernel gets per picture.  It restates the product's planning, not the
reference: what is right is decided by the oracle; this module only says which code a geometry reaches, so that the
tests can name the branch a case is there for.

The restatement is checked on the CPU: tests/test_inv_plan_host.py compares it with the launcher's own plan (inv_sbt_plan through
dsvg_inv_plan, no device needed) over the matrix, the sweep's classes and a sample of the sweep's domain.  The GPU module
(tests/test_gpu_inv_paths.py) checks that the kernels then ran as planned.

Every rule names the function or the plan step it restates (csrc/k_sbt.hip unless another file is named).
"""
import collections
import re

IT_TX, IT_TY = 16, 8          # level-3 cells per tile of the inverse kernels (k_sbt.hip, IT_TX / IT_TY)
BT_CX, BT_CY = 60, 32         # level-1 cells per tile of k_inv_b4t (k_sbt.hip, BT_CX / BT_CY)
BORDER = 64                   # DSVG_BORDER: the reference frame's border (dsvg_kernels.hpp)
FORMATS = {"444": 0x0, "422": 0x4, "420": 0x5, "411": 0x8}

# kernel names exactly as DSVG_KERNEL_IDS spells them (dsvg_host.hpp)
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
    """SbtGeo of the three planes as a context builds them (make_ctx_geo, dsvg_pipe.hip)"""
    hs, vs = (fmt >> 2) & 3, fmt & 3                                       # fmt_hs / fmt_vs (dsvg_host.hpp)
    cw, ch = rsu(w, hs), rsu(h, vs)                                        # make_frame_layout (dsvg_common.hip)
    out = []
    for c in range(3):
        pw, ph = (cw, ch) if c else (w, h)
        pstride = (pw + 2 * BORDER + 15) & ~15                             # make_frame_layout: the row stride
        W, H = ((cw + 1) & ~1, (ch + 1) & ~1) if c else (w, h)             # make_coef_layout: chroma rounded up to even (dsvg_common.hip)
        w3, h3, w2, h2, w1, h1 = rsu(W, 3), rsu(H, 3), rsu(W, 2), rsu(H, 2), rsu(W, 1), rsu(H, 1)
        # l1a (make_ctx_geo): scan regions 7..9 of make_hz_plane (dsvg_common.hip) -- the level-1 bands -- start and
        # run in multiples of 4 cells.  Region 7 starts behind LL3 and the six level-3 / level-2 detail bands.
        base7 = 4 * w3 * h3 + 3 * w2 * h2
        l1a = ((w1 | base7 | (base7 + w1 * h1) | (base7 + 2 * w1 * h1)) & 3) == 0
        out.append(Geo(W, H, pw, ph, pstride, w3, h3, rsu(W, 5), rsu(H, 5), l1a))
    return out


def fuses_border(G):
    """inv_sbt_plan's fb for the encoder's P chroma (insym = patch_kernel = fuse_border = 1), without the A/B switches: the patch
    step takes both planes whole (stated here from the planes, as chroma_p's tcx / tcy) and inv_sbt_fuses_border's alignment and
    ratio conditions hold: (fb, hr, vr)"""
    g, gy = G[1], G[0]
    for q in (G[1], G[2]):
        if q.pw != g.pw or q.ph != g.ph or q.w3 != g.w3 or q.h3 != g.h3 or q.pw & 15 or q.pstride & 15:     # inv_sbt_fuses_border: both planes alike, 16-byte rows
            return False, 0, 0
        fullc, fullr = q.pw // 8, q.ph // 8                                                                # the whole patches of a plane
        part4 = fullr == q.h3 - 1 and fullr >= 1 and (q.ph & 7) == 4 and (q.H & 7) == 4                   # the four-row last patch row
        if fullc < q.w3 or not (fullr >= q.h3 or part4):                                                   # the patch step takes the plane whole
            return False, 0, 0
    if g.pw < 16 or g.ph < 8 or gy.pw % g.pw or gy.ph % g.ph or gy.pstride & 15 or gy.pw & 15:           # inv_sbt_fuses_border: the luma plane a multiple
        return False, 0, 0
    hr, vr = gy.pw // g.pw, gy.ph // g.ph                                                                  # inv_sbt_fuses_border: hr, vr
    return (hr in (1, 2, 4) and vr in (1, 2)), hr, vr                                                      # inv_sbt_fuses_border: the ratios


def _add(k, name, nbytes):
    n, b = k.get(name, (0, 0.0))
    k[name] = (n + 1, b + nbytes)


def luma_p(g, k):
    """inv_sbt_plan, luma of a P picture from the symbol planes with the patch kernel (insym = patch_kernel = 1, filt): the
    k_inv_p_tile step and the strips step, or the whole-plane step.  Returns the branch."""
    tgx, tgy = -(-g.w3 // IT_TX), -(-g.h3 // IT_TY)                                                         # the tile grid (tgx, tgy)
    smp = float(g.W * g.H)                                                                                 # smp (nz = 1)
    fx = (g.w3 - IT_TX - 2) // IT_TX + 1 if g.l1a and g.w3 >= IT_TX + 2 else 0                              # fx
    fy = (g.h3 - IT_TY - 2) // IT_TY + 1 if g.l1a and g.h3 >= IT_TY + 2 else 0                              # fy
    if fx > 0 and fy > 0:                                                                                  # the fast-tile branch
        er = fx == tgx - 1 and g.w3 == tgx * IT_TX and (g.W & 7) == 0                                       # er
        eb = fy == tgy - 1 and (g.H & 7) == 0                                                               # eb
        fxg, fyg = fx + er, fy + eb                                                                         # fxg, fyg
        fsmp = 64.0 * min(fxg * IT_TX, g.w3) * min(fyg * IT_TY, g.h3)                                       # fsmp
        _add(k, KP_TILE_F, fsmp * 2.5)                                                                      # the k_inv_p_tile step
        nrest = (tgx - fxg) * tgy + fxg * (tgy - fyg)                                                       # the strips step's grid
        if nrest > 0:
            _add(k, KPIX_SYM_F, (smp - fsmp) * 2.5)                                                         # the strips step
        return dict(kind="fast", fx=fx, fy=fy, er=er, eb=eb, fxg=fxg, fyg=fyg, nrest=nrest, l1a=g.l1a,
                    strip_cols=tgx - fxg, strip_rows=tgy - fyg)
    _add(k, KPIX_SYM_F, smp * 2.5)                                                                          # the whole-plane step
    return dict(kind="general", l1a=g.l1a, fx=fx, fy=fy)


def chroma_p(G, k):
    """inv_sbt_plan, both chroma planes of a P picture in one launch (c0 = 1, npl = 2, insym = patch_kernel = 1, no filter): the
    k_inv_patch_c step and the strips step.  Returns the branch."""
    g = G[1]
    nz = 2
    tgx, tgy = -(-g.w3 // IT_TX), -(-g.h3 // IT_TY)
    smp = float(g.W * g.H * nz)
    fullc, fullr = g.pw // 8, g.ph // 8                                                                     # fullc, fullr
    part4 = fullr == g.h3 - 1 and fullr >= 1                                                                # part4
    part4 = part4 and all(q.ph == g.ph and (q.ph & 7) == 4 and (q.H & 7) == 4 and q.h3 == g.h3 for q in G[1:])   # part4: every plane of the launch
    tcx = tgx if fullc >= g.w3 else fullc // IT_TX                                                          # tcx, tcy
    tcy = tgy if (fullr >= g.h3 or part4) else fullr // IT_TY
    imax = g.w3 if tcx >= tgx else tcx * IT_TX                                                              # imax, jmax
    jmax = g.h3 if tcy >= tgy else tcy * IT_TY
    if imax > 0 and jmax > 0:                                                                               # the k_inv_patch_c step
        _add(k, KPATCH_C, 64.0 * imax * jmax * nz * 2.0)
    nrest = 0
    if tcx < tgx or tcy < tgy:                                                                              # the strips step
        _add(k, KPIX_SYM, (smp - 64.0 * imax * jmax * nz) * 2.5)
        nrest = (tgx - tcx) * tgy + tcx * (tgy - tcy)                                                       # the strips step's grid
    fb, hr, vr = fuses_border(G)                                                                           # InvPlan.fb (enqueue_recon reads it)
    return dict(imax=imax, jmax=jmax, part4=part4, tcx=tcx, tcy=tcy, right_strip=tcx < tgx, bottom_strip=tcy < tgy,
                nrest=nrest, fb=fb, hr=hr if fb else 0, vr=vr if fb else 0)


def intra(G, k):
    """inv_sbt_plan of an I picture from the symbol planes (insym = 1), luma then chroma: the level-3..2 step and the k_inv_b4t step"""
    for c0, npl in ((0, 1), (1, 2)):
        g = G[c0]
        smp = float(g.W * g.H * npl)
        _add(k, KS1_SYM_F if c0 == 0 else KS1_SYM, smp * 1.4)                                               # the level-3..2 step
        _add(k, KB4T_SYM, smp * 3.5)                                                                        # the k_inv_b4t step


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
        # the encoder (code_batch_impl, dsvg_pipe.hip): k_tail_q did the inverse tail (tail_done), levels 5..4 of all planes in one
        # launch (enqueue_recon; launch_inv54_all), lazy borders on
        self.p_kernels, self.i_kernels = {}, {}
        for k in (self.p_kernels, self.i_kernels):
            _add(k, K54_ALL, s3 * 8.0)
        intra(G, self.i_kernels)
        # P pictures: symY = symC = patch kernel = 1 (enqueue_recon(.., 7, ..))
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
    """the HZCC scan regions of luma or chroma overlap (dsvg_ctx_create_blk, dec_ov): a shared cell can be quantised to 0 in the
    encoder's second pass while the decoder keeps the first symbol -- the reference's decoder then drifts from its encoder's
    reconstruction (tests/test_gpu_stream.py, _decode_and_compare)"""
    for g in plane_geos(w, h, fmt)[:2]:
        sw, sh = [rsu(g.W, 3 - l) for l in range(3)], [rsu(g.H, 3 - l) for l in range(3)]
        if 2 * sw[0] > sw[1] or 2 * sh[0] > sh[1] or 2 * sw[1] > sw[2] or 2 * sh[1] > sh[2]:
            return True
    return False


def coded_geometry(w, h):
    """what dsvg_ctx_create accepts: luma at least 32x32 (dsvg_geom_check), even"""
    return w >= 32 and h >= 32 and not (w | h) & 1


def sweep_domain(wmax=1300, hmax=760):
    """every even (w, h) the encoder accepts up to wmax x hmax"""
    for h in range(32, hmax + 1, 2):
        for w in range(32, wmax + 1, 2):
            yield w, h


def sweep(wmax=1300, hmax=760, keep=3):
    """{class: the `keep` smallest geometries (w, h, fmt) of the class by area} over the sweep's domain, in all four formats"""
    seen = {}
    for fmt in FORMATS.values():
        for w, h in sweep_domain(wmax, hmax):
            c = Plan(w, h, fmt).cls
            k = seen.setdefault(c, [])
            if len(k) < keep or w * h < k[-1][0]:
                k.append((w * h, w, h, fmt))
                k.sort()
                del k[keep:]
    return {c: [g[1:] for g in k] for c, k in seen.items()}


# the op-level twin (dsvg_op_inv_sbt, dsvg_ops.hip) calls launch_inv_sbt(.., isP) with the defaults insym = 0, with_tail = 1
# (dsvg_kernels.hpp): the plan's tail step, its levels 5..4 step per plane, then the int32-coefficient steps, luma (filt) and
# chroma alike; tests/test_gpu_ops.py::test_fwd_inv_sbt drives it with c = 0 and 1
TWIN_KERNELS = {KTAIL, K54_F, K54, KPIX_F, KPIX, KS1_F, KS1, KB4T}

# inverse kernel ids no matrix case reaches, and why
UNREACHABLE = {
    KP_TILE: "k_inv_p_tile<false> needs insym with patch_kernel and no filter, but every unfiltered plane (chroma) with "
             "patch_kernel takes k_inv_patch_c first (inv_sbt_plan: the patch branch comes before the fast-tile branch)",
}
