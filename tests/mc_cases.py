"""Motion fields BUILT for the four motion-compensation kernels (k_mc in csrc/k_bmc.hip; k_fwd_mc_fast, k_fwd_mc_pix and k_mc_patch in
csrc/k_sbt.hip), and the path every (block, plane) of such a field takes, computed here from the facts the kernels branch on.  No GPU.

build_field(geo, recipe, seed) walks the blocks in raster order and gives block k a combination that differs from its neighbours':
  phase   the low bits of both vector components: bit 0 is luma's half-pel phase, bit hs (vs) is chroma's -- all sixteen combinations,
          negative odd vectors among them (the shifts are arithmetic, as in bmc.c);
  reach   per axis one of REACH: nothing, a few pixels, the position that lands one inside / exactly on / one beyond each clamp limit
          (-64 and plane size - block size + 63; stated for luma and, separately, for chroma: the chroma limits are not the luma limits
          shifted when the plane size is odd), and the ends of int16;
  mode    two inter blocks, then an intra block whose submask runs through 1 .. 15.

Two facts of the reference bound a field, and build_field enforces both:
  * an intra block with a partial submask divides by (cw / 2) * (ch / 2) (bmc.c:176-189, orc_bmc.c:61-66): where a block's clipped size
    is below 2 in either direction in ANY plane, the block gets submask 0xF;
  * a block clamped to the top limit reads row -65 (luma, vertical phase), in front of the frame's allocation, and one clamped to the
    bottom limit reads row ph + 64: the next plane's first row for Y and U, but behind the allocation for V.  Such output pixels are
    UNPINNED (unpinned_masks): the reference's answer for them is whatever its heap holds, so the tests leave them out and compare
    everything else.  build_field lets them occur in the first block row of luma and the last block row of V only (a recipe with
    pinned=True: nowhere) and pulls the vector of any other such block two pixels inside the limit.

What the product holds there.  The operators upload a host frame verbatim into a slab of its own (dsvg_ops.hip: upload_frame ->
Slab::alloc): 256 KiB of zeroed guard (GUARD_BYTES) in front, the frame, at least 4096 zeroed bytes and another 256 KiB of zeroed guard
behind.  A context keeps its reconstructions in ONE slab (csrc/dsvg_ctx_mem.h: CM_RECON, n_recon * pitch bytes + 4096 between two
256 KiB guards), slot i at i * pitch with pitch = frame bytes rounded up to 256: in front of slot i lies slot i - 1's V plane (its bottom
border and the rounding bytes), behind it slot i + 1's luma top border; the first and the last slot have the zeroed guard.  A row of the
widest plane a context takes is far below 256 KiB, so the reads one row outside a frame stay inside the slab: safe, but their value is
another picture's -- not the reference's heap, hence "unpinned" and not "zero".

Path classes (the ledger of test_mc_cases_host.py), per (block, plane), for k_mc:
  row-{copy,lumaH,chromaH}-shb{0..3}   mode 0, no vertical phase: one reference row per output row, read as three dwords around the
                                       unaligned address; shb = its low two bits = (wx - 1) & 3 (plane offsets and strides are
                                       multiples of 4, the slabs 256-aligned)
  window-V, window-HV, window-chroma-V, window-chroma-HV
  intra-lean-w{16,32,64}-{all,partial}      whole block, 16 / 32 / 64 wide in ITS plane, even height of whole row passes
  intra-window-{whole,clipped-even,clipped-odd}-{all,partial}
and for the fused geometries fast / pix / list from the product's own plans (decode_plan, code_batch_plan) with fwd_fast_sel
(k_sbt.hip:872-891) restated in fast_sel()."""
import numpy as np

import _cabi as A

BORDER = A.BORDER
REACH = ("zero", "small+", "small-",
         "L-lo-in", "L-lo-at", "L-lo-out", "L-hi-in", "L-hi-at", "L-hi-out",
         "C-lo-in", "C-lo-at", "C-lo-out", "C-hi-in", "C-hi-at", "C-hi-out",
         "max", "-max", "min", "small2")
RECIPES = {                                     # intra: every third block; kinds: the reaches used; pinned: no unpinned pixel anywhere
    "full": dict(intra=True, kinds=REACH, pinned=False),
    "full-pinned": dict(intra=True, kinds=REACH, pinned=True),
    "inter": dict(intra=False, kinds=REACH, pinned=False),
    "inter-pinned": dict(intra=False, kinds=REACH, pinned=True),
    "zero": dict(intra=False, kinds=("zero",), pinned=True, phases=False),
    "reach5": dict(intra=False, kinds=("reach5+", "reach5-"), pinned=True, phases=False),
    "beyond": dict(intra=False, kinds=("L-lo-out", "L-hi-out", "C-lo-out", "C-hi-out", "max", "-max", "min"), pinned=True),
}


class Geo:
    """a picture, its block grid and the frame layout of frame.c:63-120 (the same numbers as _cabi.BorderedFrame and make_frame_layout)"""

    def __init__(self, w, h, fmt, bw=None, bh=None):
        if bw is None:
            bw, bh = A.block_dims(w, h)[:2]
        self.w, self.h, self.fmt, self.bw, self.bh = w, h, fmt, bw, bh
        self.nbh, self.nbv = -(-w // bw), -(-h // bh)
        self.nblk = self.nbh * self.nbv
        self.hs, self.vs = A.hshift(fmt), A.vshift(fmt)
        f = A.BorderedFrame(w, h, fmt)
        self.dims, self.strides, self.total = f.dims, f.strides, f.total
        self.offs = [o - f.GUARD for o in f.offs]                  # of pixel (0, 0) of each plane from the allocation's first byte
        self.name = "%dx%d-%s-b%dx%d" % (w, h, {0: "444", 4: "422", 5: "420", 8: "411"}[fmt], bw, bh)

    def shifts(self, c):
        return (self.hs, self.vs) if c else (0, 0)

    def blk(self, c):
        sh, sv = self.shifts(c)
        return self.bw >> sh, self.bh >> sv

    def lim(self, c):
        """upper clamp limits (x, y) of plane c; the lower ones are -64"""
        bw, bh = self.blk(c)
        return self.dims[c][0] - bw + BORDER - 1, self.dims[c][1] - bh + BORDER - 1

    def block(self, c, i, j):
        """(x, y, cw, ch) of block (i, j) in plane c, or None where the plane has no such block"""
        bw, bh = self.blk(c)
        pw, ph = self.dims[c]
        x, y = i * bw, j * bh
        if x >= pw or y >= ph:
            return None
        return x, y, (pw - x if x + bw >= pw else bw), (ph - y if y + bh >= ph else bh)

    def fusable(self):
        """mc_fusable (k_sbt.hip)"""
        return (self.bw >> self.hs) % 8 == 0 and (self.bh >> self.vs) % 8 == 0 and self.bw % 8 == 0 and self.bh % 8 == 0


def _clampi(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def placed(geo, c, i, j, mvx, mvy):
    """(wx, wy, xh, yh, prex, prey) of an inter block in plane c: the clamp of k_bmc.hip:99-102 / orc_bmc.c:88-90; pre* before the clamp"""
    sh, sv = geo.shifts(c)
    x, y, _, _ = geo.block(c, i, j)
    dx, dy = int(mvx) >> sh, int(mvy) >> sv
    lx, ly = geo.lim(c)
    px, py = x + (dx >> 1), y + (dy >> 1)
    return _clampi(px, -BORDER, lx), _clampi(py, -BORDER, ly), dx & 1, dy & 1, px, py


def _axis(kind, bits, pos_l, pos_c, lim_l, lim_c, s, n):
    """one vector component: reach `kind`, phase bits (bit 0 luma, bit 1 chroma), block position and upper limit in luma / chroma"""
    pl, pc = bits & 1, (bits >> 1) & 1
    def both(d):                                     # d pixels of the chroma plane, both phases as asked
        return (d << (s + 1)) | (pc << s) | pl if s else (d << 1) | pl
    rel = {"in": 1, "at": 0, "out": -1}
    if kind == "zero":
        v = 0
    elif kind in ("small+", "small-", "small2"):
        d = 1 + n % 5
        v = both(d if kind == "small+" else -d - (kind == "small2"))
    elif kind in ("reach5+", "reach5-"):
        v = 10 if kind == "reach5+" else -10
    elif kind == "max":
        v = 32767
    elif kind == "-max":
        v = -32767
    elif kind == "min":
        v = -32768
    else:
        plane, side, r = kind.split("-")
        lim, pos = (lim_l, pos_l) if plane == "L" else (lim_c, pos_c)
        t = -BORDER + rel[r] if side == "lo" else lim - rel[r]
        v = 2 * (t - pos) + pl if plane == "L" else both(t - pos)
    return _clampi(v, -32768, 32767)


def unpinned_block(geo, c, i, j, mv):
    """bool (ch, cw): output pixels of block (i, j) of plane c whose taps include a byte outside the frame's own allocation"""
    x, y, cw, ch = geo.block(c, i, j)
    out = np.zeros((ch, cw), dtype=bool)
    if mv["mode"] != 0:
        return out
    wx, wy, xh, yh, _, _ = placed(geo, c, i, j, mv["x"], mv["y"])
    lo, hi = (-1, 2) if c == 0 else (0, 1)           # luma: four taps m a b p around a; chroma: a and its neighbour
    c0, c1 = (lo, hi) if xh else (0, 0)
    r0, r1 = (lo, hi) if yh else (0, 0)
    st = geo.strides[c]
    yy, xx = np.arange(ch)[:, None], np.arange(cw)[None, :]
    first = geo.offs[c] + (wy + yy + r0) * st + wx + xx + c0
    last = geo.offs[c] + (wy + yy + r1) * st + wx + xx + c1
    return (first < 0) | (last >= geo.total)


def unpinned_masks(geo, mv):
    """per plane a bool (h, w): True = left out of every comparison"""
    out = [np.zeros((d[1], d[0]), dtype=bool) for d in geo.dims]
    for c in range(3):
        for j in range(geo.nbv):
            for i in range(geo.nbh):
                b = geo.block(c, i, j)
                m = mv[j * geo.nbh + i]
                if b is None or m["mode"] != 0:
                    continue
                x, y, cw, ch = b
                wy = placed(geo, c, i, j, m["x"], m["y"])[1]
                if wy - 1 <= -BORDER or wy + ch + 2 >= geo.dims[c][1] + BORDER - 1:     # (only the outermost rows can leave the frame)
                    out[c][y:y + ch, x:x + cw] = unpinned_block(geo, c, i, j, m)
    return out


def _allowed_unpinned(geo, c, j, pinned):
    return not pinned and ((c == 0 and j == 0) or (c == 2 and j == geo.nbv - 1))


def build_field(geo, recipe, seed):
    """-> (field of A.MV_DTYPE, tags): tags[c][blk] = the list of classes of (blk, plane c) (classify), None where the plane lacks the block"""
    R = RECIPES[recipe]
    kinds = R["kinds"]
    mv = np.zeros(geo.nblk, dtype=A.MV_DTYPE)
    n = seed * 7                                      # counts the inter blocks, ni the intra ones
    ni = seed * 4
    limx_l, limy_l = geo.lim(0)
    limx_c, limy_c = geo.lim(1)
    for j in range(geo.nbv):
        for i in range(geo.nbh):
            k = j * geo.nbh + i
            if R["intra"] and (k + seed) % 3 == 2:
                sub = 1 + ni % 15
                ni += 1
                # the reference divides by (cw / 2) * (ch / 2): no partial submask where that is zero in any plane
                if any(b is not None and (b[2] < 2 or b[3] < 2) for b in (geo.block(c, i, j) for c in range(3))):
                    sub = 0xF
                mv[k]["mode"], mv[k]["submask"] = 1, sub
                continue
            ph = n % 16 if R.get("phases", True) else 0
            kx, ky = kinds[n % len(kinds)], kinds[(n + n // len(kinds) + 5 * seed) % len(kinds)]
            bc = geo.block(1, i, j) or (i * (geo.bw >> geo.hs), j * (geo.bh >> geo.vs), 0, 0)
            vx = _axis(kx, ph & 3, i * geo.bw, bc[0], limx_l, limx_c, geo.hs, n)
            vy = _axis(ky, ph >> 2, j * geo.bh, bc[1], limy_l, limy_c, geo.vs, n // 5)
            mv[k]["x"], mv[k]["y"] = vx, vy
            # unpinned pixels only where they are allowed: elsewhere the vertical component moves inside the limits
            bad = [c for c in range(3) if geo.block(c, i, j) is not None and not _allowed_unpinned(geo, c, j, R["pinned"])
                   and unpinned_block(geo, c, i, j, mv[k]).any()]
            if bad:
                # (two inside: a corner tap of the row next to the limit leaves the frame by one byte where the block is clamped sideways too)
                lo = 2 * (-BORDER + 2 - j * geo.bh)
                hi = (2 * (limy_c - 2 - bc[1])) << geo.vs
                mv[k]["y"] = _clampi(vy, lo, min(hi, 2 * (limy_l - 2 - j * geo.bh)))
                assert not any(unpinned_block(geo, c, i, j, mv[k]).any() for c in bad), (geo.name, i, j, vy)
            n += 1
    return mv, classify(geo, mv)


def _rel(pre, lo, hi):
    """side and relation of an unclamped position to the limits: in (one inside), at, out (one beyond), far; None away from them"""
    for side, d in (("lo", lo - pre), ("hi", pre - hi)):
        if d >= -1:
            return side, {-1: "in", 0: "at", 1: "out"}.get(d, "far")
    return None


def classify(geo, mv):
    """tags[c][blk]: first the k_mc path class, then lean-sub<n> / window-sub<n> of an intra block and clamp-{luma,chroma}-{L,R,T,B}-{in,at,
    out,far} of an inter block whose unclamped position lies within one pixel of a limit or beyond it"""
    tags = [[None] * geo.nblk for _ in range(3)]
    for c in range(3):
        bw, bh = geo.blk(c)
        kind = "luma" if c == 0 else "chroma"
        for j in range(geo.nbv):
            for i in range(geo.nbh):
                b = geo.block(c, i, j)
                if b is None:
                    continue
                x, y, cw, ch = b
                m = mv[j * geo.nbh + i]
                t = []
                if m["mode"] == 0:
                    wx, wy, xh, yh, px, py = placed(geo, c, i, j, m["x"], m["y"])
                    if not yh:
                        t.append("row-%s-shb%d" % ("copy" if not xh else ("lumaH" if c == 0 else "chromaH"), (wx - 1) & 3))
                    else:
                        t.append("window-%s%s" % ("" if c == 0 else "chroma-", "HV" if xh else "V"))
                    lx, ly = geo.lim(c)
                    for pre, hi, sides in ((px, lx, "LR"), (py, ly, "TB")):
                        r = _rel(pre, -BORDER, hi)
                        if r:
                            t.append("clamp-%s-%s-%s" % (kind, sides[r[0] == "hi"], r[1]))
                else:
                    sub = int(m["submask"])
                    part = "all" if sub == 0xF else "partial"
                    rpp = {16: 16, 32: 8, 64: 4}.get(bw)                 # rows per pass of the lean body (k_bmc.hip:167-172)
                    if rpp and cw == bw and ch == bh and bh % rpp == 0 and bh // rpp <= 16 and not (ch & 1) and geo.strides[c] % 4 == 0:
                        t += ["intra-lean-w%d-%s" % (bw, part), "lean-%s-sub%d" % (kind, sub), "lean-sub%d" % sub]
                    else:
                        shape = "whole" if cw == bw and ch == bh else ("clipped-odd" if (cw | ch) & 1 else "clipped-even")
                        t += ["intra-window-%s-%s" % (shape, part), "window-sub%d" % sub]
                tags[c][j * geo.nbh + i] = t
    return tags


def explain(geo, mv, tags, c, got, want, mask, what, fused=None):
    """AssertionError text for plane c (got / want (h, w), mask True = compared), or None where they agree: plane, block, vector, mode,
    path class and the first differing pixel; fused(c, x, y): the kernel of the fused geometries that wrote the pixel"""
    bad = (np.asarray(got) != np.asarray(want)) & mask
    if not bad.any():
        return None
    ys, xs = np.nonzero(bad)
    y, x = int(ys[0]), int(xs[0])
    bw, bh = geo.blk(c)
    i, j = x // bw, y // bh
    m = mv[j * geo.nbh + i]
    return ("%s %s: plane %d differs at %d pixels; first (x %d, y %d) got %d want %d: block (%d, %d) vector (%d, %d) mode %d submask %d, "
            "path %s%s" % (geo.name, what, c, int(bad.sum()), x, y, int(got[y, x]), int(want[y, x]), i, j, int(m["x"]), int(m["y"]),
                           int(m["mode"]), int(m["submask"]), " ".join(tags[c][j * geo.nbh + i]), " " + fused(c, x, y) if fused else ""))


def raw_mask(geo, unp):
    """bool over a BorderedFrame's raw(): False at the interior pixels that `unp` leaves out"""
    keep = np.ones(geo.total, dtype=bool)
    for c in range(3):
        ys, xs = np.nonzero(unp[c])
        keep[geo.offs[c] + ys * geo.strides[c] + xs] = False
    return keep


# ---- the float reciprocal of k_fwd_mc_fast (k_sbt.hip:917-918) ---------------------------------------------------------------------
def fast_block_index(I, n, ulp=0):
    """(int)((I + 0.5f) * rcp(n)) in float32: rcp correctly rounded, or one ulp below (-1) / above (+1) as v_rcp_f32 may be"""
    r = np.float32(1) / np.float32(n)
    if ulp:
        r = np.nextafter(r, np.float32(2 if ulp > 0 else 0), dtype=np.float32)
    return ((np.asarray(I).astype(np.float32) + np.float32(0.5)) * r).astype(np.int32)


# ---- fwd_fast_sel (k_sbt.hip:872-891) ----------------------------------------------------------------------------------------------
def fast_sel(lv, nb, I, J, x0, y0, pw, ph):
    """does patch (I, J) of a plane take k_fwd_mc_fast (True) or k_fwd_mc_pix?  sparse P picture assumed; lv = [(w, h)] of the scan
    regions of levels 3, 2, 1 (hzcc.c:30-48: the plane's size halved with rounding up), nb = (nbh, nbv) of the stability map.
    QLevel.dbx / dby are the 14-bit fixed-point block steps of hzcc.c:196-197: (nb << 14) / region size."""
    (w3, h3), (w2, h2), (w1, h1) = lv
    ovx = 2 * w3 > w2 or 2 * w2 > w1
    ovy = 2 * h3 > h2 or 2 * h2 > h1
    if not (x0 + 8 <= pw and y0 + 8 <= ph) or (ovx and I == 0) or (ovy and J == 0):
        return False
    d1, d2 = (nb[0] << 14) // w1, (nb[0] << 14) // w2
    return (4 * I * d1) >> 14 == ((4 * I + 3) * d1) >> 14 and (2 * I * d2) >> 14 == ((2 * I + 1) * d2) >> 14


def levels(pw, ph):
    """scan-region sizes of levels 3, 2, 1 of a plane whose coefficient plane is pw x ph"""
    out = []
    for s in (3, 2, 1):
        out.append((A.rshift_up(pw, s), A.rshift_up(ph, s)))
    return out


# ---- the case table ----------------------------------------------------------------------------------------------------------------
OP_BLOCKS = ((16, 16), (24, 16), (32, 32), (48, 32), (64, 64), (64, 16), (16, 64))
OP_FRAMES = ((200, 136), (203, 135))
OP_FMTS = (A.SUBSAMP_420, A.SUBSAMP_422, A.SUBSAMP_444, A.SUBSAMP_411)


def op_cases():
    """(Geo, recipe, seed) of the operator level: dsvg_params.blk_w / blk_h are the caller's there"""
    out, seed = [], 0
    for (w, h) in OP_FRAMES:
        for fmt in OP_FMTS:
            for (bw, bh) in OP_BLOCKS:
                out.append((Geo(w, h, fmt, bw, bh), "full", seed))
                seed += 1
    # a picture whose last block column is ONE pixel wide in chroma (the division-by-zero rule) and odd in luma; all inter on the odd one
    out.append((Geo(193, 130, A.SUBSAMP_420, 16, 16), "full", 3))
    out.append((Geo(203, 135, A.SUBSAMP_420, 16, 16), "inter", 11))
    out.append((Geo(200, 136, A.SUBSAMP_444, 64, 64), "full", 5))        # more 64-wide chroma intra blocks
    out.append((Geo(200, 136, A.SUBSAMP_444, 64, 64), "full", 9))
    return out


def min_picture_width(bw_want, h=64):
    """the smallest even width for which A.block_dims gives block width bw_want"""
    w = 16
    while A.block_dims(w, h)[0] != bw_want:
        w += 2
    return w


W32, W64 = min_picture_width(32), min_picture_width(64)          # 706 and 1282

CTX_GEOMS = (                                   # context level, in the product's own block size
    (96, 64, A.SUBSAMP_420),                    # 16x16 blocks, fused, every patch whole
    (250, 130, A.SUBSAMP_420),                  # ragged patches, shared scan cells, ex0 / ey0 inside the picture, cw_extra in chroma
    (384, 240, A.SUBSAMP_420),                  # 24x16 blocks: plain k_mc
    (352, 288, A.SUBSAMP_444),
    (320, 240, A.SUBSAMP_422),
    (W32, 64, A.SUBSAMP_420),                   # 32-wide blocks
    (W64, 64, A.SUBSAMP_420),                   # 64-wide blocks
)
WIDE = (8832, 64, A.SUBSAMP_420)                # 1104 luma patches a row: the largest I of the reciprocal


def ctx_cases():
    """(Geo, recipe, seed) of the context level; the wide picture with no unpinned pixel (its rows are longer than a host frame's guard)"""
    out = [(Geo(w, h, fmt), "full", 20 + n) for n, (w, h, fmt) in enumerate(CTX_GEOMS)]
    out.append((Geo(*WIDE), "full-pinned", 40))
    return out


def all_cases():
    return op_cases() + ctx_cases()


# ---- the fused geometries: who takes a block / a patch, from the product's own plans ------------------------------------------------
def list_blocks(geo, mv, ex0, ey0):
    """the blocks k_mc takes by list beside k_mc_patch (decoder; ex0 / ey0 of dsvg_decode_plan): intra, or in a block column / row from
    (ex0, ey0) on -- the predicate dec_intra_list and k_mc_patch share (dsvg_dec_plan.h:95-103)"""
    b = np.arange(geo.nblk)
    return np.nonzero((mv["mode"] != 0) | (b % geo.nbh >= ex0) | (b // geo.nbh >= ey0))[0]


def residual_entries(geo, c, seed, small=False):
    """a dozen symbols spread over the scan of plane c: (position, symbol) for _hzbits.plane_payload; small: none beyond +-2"""
    cw, ch = A.coef_dims(geo.w, geo.h, geo.fmt, c)
    rng = np.random.default_rng(seed * 3 + c)
    pos = np.unique(rng.integers(1, cw * ch, 12))
    return [(int(p), int(s)) for p, s in zip(pos, rng.choice([-2, -1, 1, 2] if small else [-3, -2, -1, 1, 2, 4], pos.size))]


def enc_paths(geo, mv):
    """{'fast': n, 'pix': n, 'list': n} of an encoder field on a fused geometry: patches per kernel over the three planes (fast_sel; the
    patches of intra blocks take either kernel too, behind k_mc's residual) and the blocks k_mc takes by list (the intra ones: ilist of
    dsvg_code_batch_plan)"""
    n = {"fast": 0, "pix": 0, "list": int((mv["mode"] != 0).sum())}
    for c in range(3):
        pw, ph = geo.dims[c]
        cw, ch = A.coef_dims(geo.w, geo.h, geo.fmt, c)
        lv = levels(cw, ch)
        for J in range(lv[0][1]):
            for I in range(lv[0][0]):
                n["fast" if fast_sel(lv, (geo.nbh, geo.nbv), I, J, 8 * I, 8 * J, pw, ph) else "pix"] += 1
    return n


def enc_kernel_of(geo, mv):
    """fused(c, x, y) for explain(): the encoder kernel that predicts pixel (x, y) of plane c on a fused geometry"""
    def f(c, x, y):
        bw, bh = geo.blk(c)
        cw, ch = A.coef_dims(geo.w, geo.h, geo.fmt, c)
        fast = fast_sel(levels(cw, ch), (geo.nbh, geo.nbv), x // 8, y // 8, x & ~7, y & ~7, *geo.dims[c])
        intra = mv[(y // bh) * geo.nbh + x // bw]["mode"] != 0
        return "[%s%s]" % ("list, then " if intra else "", "fast" if fast else "pix")
    return f


def dec_kernel_of(geo, mv, ex0, ey0):
    """fused(c, x, y) for explain(): the decoder kernel that predicts pixel (x, y) of plane c where k_mc_patch runs"""
    listed = set(list_blocks(geo, mv, ex0, ey0).tolist())

    def f(c, x, y):
        bw, bh = geo.blk(c)
        return "[list]" if (y // bh) * geo.nbh + x // bw in listed else "[patch]"
    return f
