"""Picture pairs BUILT for the branches of the motion search (csrc/k_hme.hip `hme_block`), one pair of frames per pyramid level.  No GPU.

The operator seam takes the block size from the caller and a source and a reference frame of its own for every level, so a level's
pictures here are independent frames: level l + 1 is not a reduction of level l, it is whatever sends the wanted parents to level l.
Builders write PIXELS, never vectors; which labels of hme_plan.LABELS a built pair reaches is decided by the oracle's trace
(test_hme_cases_host.py proves that every case reaches the labels it lists), and every builder that draws noise takes a seed.

The builders:
  flat      every level flat: source value a, reference value b (every SAD of a stage ties)
  field     a reference of texture at every level and a source whose blocks are cut out of it at a vector of their own: twice the
            parent block's vector plus a step of -1 / 0 / +1 per axis drawn per block (so the search can follow it), at the levels named;
            at level 0 a block may instead sit at the zero vector (it then wins from outside the parents' box) or be cut out of one of
            the eight half-pel planes of the reference (so that this half-pel candidate has SAD 0)
  mix       level 0 only, no motion: every block draws a kind of source block (flat at a value around the 2^32 wrap of sum * sum, flat
            with one pixel off by one, a step, faint noise, texture), a kind of reference block (the same, shifted, flat, noise, mirrored,
            the same with a subset of its quadrants shifted) and kinds of chroma blocks: the statistics, the six intra tests, the veto, the
            vote and its sixteen submasks
  sadmax    source 0 against reference 255 at level 0 under moving upper levels: the largest SAD there is, in the candidate stage
  bias      flat partial blocks whose sums make udiv_rd's quotient exact and its rounded product fall below it

The reference divides by a partial block's chroma area and dies on blocks one pixel wide or high: no geometry here has either."""
import numpy as np

import _cabi as A
import hme_plan as P

BORDER = A.BORDER
F420, F444, F422, F411 = A.SUBSAMP_420, A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_411


def full_view(f, c):
    """plane c of a BorderedFrame with its border: (h + 128, w + 128), pixel (0, 0) at [64, 64]"""
    w, h = f.dims[c]
    s = f.strides[c]
    o = f.offs[c] - BORDER * s - BORDER
    return np.lib.stride_tricks.as_strided(f.buf[o:], shape=(h + 2 * BORDER, w + 2 * BORDER), strides=(s, 1))


def extend(f, c):
    """replicate plane c's edge pixels into its border (frame.c:263-327)"""
    v = full_view(f, c)
    v[:, :] = np.pad(f.plane(c), BORDER, mode="edge")


def texture(rng, kind, h, w):
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    if kind == "mid":                                  # texture that every pixel of can be coded as mean + residual
        return rng.integers(96, 161, size=(h, w)).astype(np.uint8)
    if kind == "smooth":
        base = rng.integers(0, 256, size=(h // 8 + 2, w // 8 + 2)).astype(np.float64)
        return np.clip(np.kron(base, np.ones((8, 8)))[:h, :w] + rng.integers(-6, 7, size=(h, w)), 0, 255).astype(np.uint8)
    if kind == "extreme":                              # 2x2 cells of 0 / 255: the half-pel taps reach 4590 and -510, sat8 works on both sides
        yy, xx = np.mgrid[0:h, 0:w]
        pat = ((((xx + 3) >> 1) ^ ((yy + 3) >> 1)) & 1) * 255
        cells = np.kron(rng.integers(0, 4, size=(h // 16 + 1, w // 16 + 1)), np.ones((16, 16), dtype=np.int64))[:h, :w]
        return np.where(cells > 0, pat, rng.integers(0, 256, size=(h, w))).astype(np.uint8)
    if kind == "columns":                              # constant along y: the vertical neighbours of every search point tie
        return np.repeat(rng.integers(0, 256, size=(1, w)), h, axis=0).astype(np.uint8)
    raise ValueError(kind)


def new_pair(geo, l):
    w, h = geo.dims[l]
    return A.BorderedFrame(w, h, geo.fmt), A.BorderedFrame(w, h, geo.fmt)


def blocks(geo, l):
    """the blocks level l visits: (i, j, bx, by, bw, bh) (hme.c:436-450)"""
    step = 1 << l
    fw, fh = geo.dims[l]
    for j in range(0, geo.nyb, step):
        for i in range(0, geo.nxb, step):
            bx, by = (i * geo.bw) >> l, (j * geo.bh) >> l
            if bx < fw and by < fh:
                yield i, j, bx, by, min(fw - bx, geo.bw), min(fh - by, geo.bh)


def halfpel_planes(ref):
    """the H, V and D sample planes of hpel (hme.c:350-376) of a whole bordered plane (int arrays; two pixels of margin are garbage)"""
    p = ref.astype(np.int64)
    h = np.zeros_like(p)
    h[:, 1:-2] = 9 * (p[:, 1:-2] + p[:, 2:-1]) - (p[:, :-3] + p[:, 3:])
    v = np.zeros_like(p)
    v[1:-2, :] = 9 * (p[1:-2, :] + p[2:-1, :]) - (p[:-3, :] + p[3:, :])
    d = np.zeros_like(p)
    d[1:-2, :] = 9 * (h[1:-2, :] + h[2:-1, :]) - (h[:-3, :] + h[3:, :])
    return (np.clip((h + 8) >> 4, 0, 255).astype(np.uint8), np.clip((v + 8) >> 4, 0, 255).astype(np.uint8),
            np.clip((d + 128) >> 8, 0, 255).astype(np.uint8))


def fill_chroma(rng, f, kind="noise"):
    for c in (1, 2):
        w, h = f.dims[c]
        f.plane(c)[:, :] = texture(rng, kind, h, w) if kind != "flat" else 128
        extend(f, c)


def b_flat(geo, seed, a=128, b=128):
    src, ref = [], []
    for l in range(geo.levels + 1):
        s, r = new_pair(geo, l)
        for f, v in ((s, a), (r, b)):
            for c in range(3 if l == 0 else 1):
                f.plane(c)[:, :] = v
                extend(f, c)
        src.append(s)
        ref.append(r)
    return src, ref


def b_field(geo, seed, move=(), tex="noise", canvas=False, steps=(-1, 0, 1), p_zero=0.0, halfpel=False, p_move=1.0, const=None):
    rng = np.random.default_rng(seed)
    src, ref = [None] * (geo.levels + 1), [None] * (geo.levels + 1)
    vecs = {}                                          # (level, i, j) -> the block's vector in the level's pixels
    for l in range(geo.levels, -1, -1):
        s, r = new_pair(geo, l)
        w, h = geo.dims[l]
        if canvas:                                     # the reference's border holds texture of its own
            full_view(r, 0)[:, :] = texture(rng, tex, h + 2 * BORDER, w + 2 * BORDER)
        else:
            r.plane(0)[:, :] = texture(rng, tex, h, w)
            extend(r, 0)
        rf = full_view(r, 0)
        planes = halfpel_planes(rf) if halfpel and l == 0 else None
        step = 1 << l
        for i, j, bx, by, bw, bh in blocks(geo, l):
            pi, pj = i & ~(2 * step - 1), j & ~(2 * step - 1)
            px, py = vecs.get((l + 1, pi, pj), (0, 0))
            vx, vy = 2 * px, 2 * py
            if l in move and rng.random() < p_move:
                d = const if const is not None else (int(rng.choice(steps)), int(rng.choice(steps)))
                vx, vy = vx + d[0], vy + d[1]
            if l == 0 and rng.random() < p_zero:
                vx, vy = 0, 0
            vecs[(l, i, j)] = (vx, vy)
            y0, x0 = by + vy + BORDER, bx + vx + BORDER
            cut = rf
            if planes is not None:
                k = int(rng.integers(0, 10))           # 8, 9: full-pel
                if k < 8:
                    hx, hy = P.HP[k]
                    cut = planes[0] if hy == 0 else (planes[1] if hx == 0 else planes[2])
                    x0, y0 = x0 - (hx < 0), y0 - (hy < 0)
            s.plane(0)[by:by + bh, bx:bx + bw] = cut[y0:y0 + bh, x0:x0 + bw]
        extend(s, 0)
        if l == 0:
            fill_chroma(rng, s)
            fill_chroma(rng, r)
        src[l], ref[l] = s, r
    return src, ref


def b_sadmax(geo, seed):
    src, ref = b_field(geo, seed, move=(1, 2), tex="noise")
    src[0].plane(0)[:, :] = 0
    ref[0].plane(0)[:, :] = 255
    extend(src[0], 0)
    extend(ref[0], 0)
    return src, ref


FLATS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 200, 254, 255)


def _src_block(rng, kind, bh, bw):
    if kind == "flat":
        return np.full((bh, bw), int(rng.choice(FLATS)), dtype=np.int64)
    if kind == "flat1":                                # flat, one pixel off by one: sum * sum just beside a multiple of the area
        v = int(rng.choice(FLATS[1:-1]))
        b = np.full((bh, bw), v, dtype=np.int64)
        b[int(rng.integers(0, bh)), int(rng.integers(0, bw))] += int(rng.choice((-1, 1)))
        return b
    if kind == "step":
        a, c = int(rng.integers(60, 120)), int(rng.integers(130, 190))
        b = np.full((bh, bw), a, dtype=np.int64)
        b[:, bw // 2 + int(rng.integers(-2, 3)):] = c
        return b
    if kind == "faint":
        return int(rng.integers(40, 216)) + rng.integers(-2, 3, size=(bh, bw))
    if kind == "mid":
        return rng.integers(96, 161, size=(bh, bw))
    return rng.integers(0, 256, size=(bh, bw))         # "noise"


def b_mix(geo, seed):
    rng = np.random.default_rng(seed)
    src, ref = [], []
    for l in range(geo.levels + 1):
        s, r = new_pair(geo, l)
        w, h = geo.dims[l]
        if l:
            r.plane(0)[:, :] = texture(rng, "noise", h, w)
            s.plane(0)[:, :] = r.plane(0)
        else:
            for i, j, bx, by, bw, bh in blocks(geo, 0):
                sk = str(rng.choice(("flat", "flat", "flat1", "step", "faint", "mid", "mid", "noise")))
                sb = _src_block(rng, sk, bh, bw)
                rk = str(rng.choice(("same", "shift", "flat", "noise", "mirror", "quad", "quad", "faint")))
                if rk == "same":
                    rb = sb.copy()
                elif rk == "shift":
                    rb = sb + int(rng.choice((-40, -9, -3, -2, -1, 1, 2, 3, 9, 40)))
                elif rk == "flat":
                    rb = np.full((bh, bw), int(rng.choice(FLATS)), dtype=np.int64)
                elif rk == "mirror":
                    rb = sb[:, ::-1].copy()
                elif rk == "quad":                     # the quadrants of the submask are shifted, the others the source's own (hme.c:689-716)
                    m = int(rng.integers(0, 16))
                    rb = sb.copy()
                    qw, qh = bw // 2, bh // 2
                    for q in range(4):
                        if m >> q & 1:
                            rb[(q >> 1) * qh:(q >> 1) * qh + qh, (q & 1) * qw:(q & 1) * qw + qw] += int(rng.choice((-40, 40)))
                else:
                    rb = _src_block(rng, rk, bh, bw)
                s.plane(0)[by:by + bh, bx:bx + bw] = np.clip(sb, 0, 255)
                r.plane(0)[by:by + bh, bx:bx + bw] = np.clip(rb, 0, 255)
                cbw, cbh = -(-bw >> geo.hs), -(-bh >> geo.vs)
                cx, cy = i * (geo.bw >> geo.hs), j * (geo.bh >> geo.vs)
                for c in (1, 2):
                    for f, kinds in ((s, ("flat", "flat", "faint", "noise")), (r, ("flat", "faint", "noise", "noise"))):
                        dst = f.plane(c)[cy:cy + cbh, cx:cx + cbw]
                        dst[:, :] = np.clip(_src_block(rng, str(rng.choice(kinds)), cbh, cbw), 0, 255)[:dst.shape[0], :dst.shape[1]]
            for f in (s, r):
                extend(f, 1)
                extend(f, 2)
        extend(s, 0)
        extend(r, 0)
        src.append(s)
        ref.append(r)
    return src, ref


def b_bias(geo, seed):
    """flat everywhere; at level 0 every block whose area is no power of two gets a flat reference block of a value u and a flat source block
    of a value v at most 8 away, such that (u * area)^2 / area is a division whose rounded product n * (1 / area) falls below the exact
    quotient while (v * area)^2 / area is not (both squares below 2^32).  The zero-motion variance is then 0 only with udiv_rd's bias
    (k_hme.hip:246); without it it is 1 > 2 * 0 and the block turns intra (hme.c:652-655).  Chroma is flat: no other test fires."""
    src, ref = b_flat(geo, seed, 128, 128)
    for i, j, bx, by, bw, bh in blocks(geo, 0):
        area = bw * bh
        if area & (area - 1) == 0:
            continue
        vals = [u for u in range(1, 256) if u * area < 65536]
        need = [u for u in vals if P._needs_bias((u * area) ** 2, area)]
        pairs = [(u, v) for u in need for v in vals if 0 < abs(u - v) <= 8 and v not in need]
        if pairs:
            u, v = pairs[(i + j + seed) % len(pairs)]
            src[0].plane(0)[by:by + bh, bx:bx + bw] = v
            ref[0].plane(0)[by:by + bh, bx:bx + bw] = u
    extend(src[0], 0)
    extend(ref[0], 0)
    return src, ref


BUILDERS = {"flat": b_flat, "field": b_field, "mix": b_mix, "sadmax": b_sadmax, "bias": b_bias}


class Case:
    def __init__(self, name, w, h, fmt, bw, bh, levels, builder, kw, labels, dims=None):
        self.name, self.builder, self.kw, self.labels = name, builder, kw, tuple(labels)
        self.geo = P.Geo(w, h, fmt, bw, bh, levels, dims)
        assert w <= 384 and h <= 256

    def build(self):
        return BUILDERS[self.builder](self.geo, **self.kw)

    def flags(self):
        """the operator calls of the case: plain, and with the table where level 0 has full blocks / luma in place where the geometry allows it"""
        g = self.geo
        f = (P.HME_TABLE if g.has_fast0() else 0) | (P.HME_IN_CLIP if g.in_clip_ok else 0)
        return [0, f] if f else [0]


CASES = []


def _case(*a, **kw):
    CASES.append(Case(*a, **kw))


# name, w, h, fmt, blk_w, blk_h, levels, builder, its arguments, the labels the case is there for (hme_plan.LABELS; the case usually reaches
# many more).  Sizes: the smallest at which the labels still occur -- 64x32, 64x48 and 64x64 blocks for the full-block body (with a right
# column / bottom row of 16, 4 and 49 pixels), 16 / 24 / 32 / 48-pixel blocks with ragged edges of 1 .. 13 pixels for the generic one.
_case("flat-same", 320, 192, F420, 64, 32, 2, "flat", dict(seed=0, a=128, b=128),
       ["var.luma.wrap", "bin.HP_SKIPPED", "bin.INTRA_NONE", "blk.full", "blk.partial.corner", "body.general.cmask.empty",
        "clip.src.clip", "clip.ref.ring"])
_case("flat-diff", 208, 148, F420, 64, 48, 2, "flat", dict(seed=0, a=100, b=200),
       ["var.luma.nowrap", "bin.HP_KEPT_FULLPEL", "bin.INTRA_AVG", "blk.partial.right", "blk.narrow", "part.1", "clip.ref.clip"])
_case("flat-veto", 125, 77, F444, 16, 16, 3, "flat", dict(seed=0, a=0, b=255),
       ["var.zero.nowrap", "bin.NB0_PLAIN", "bin.VETO_TAKEN", "blk.partial.bottom", "body.general.uni"])
_case("sadmax", 384, 256, F420, 64, 64, 2, "sadmax", dict(seed=1),
       ["cand.n1", "cand.dup.d3", "cand.offgrid.B", "cand.tie", "cand.sadmax", "part.3", "win.spy_exact", "win.mis3"])
_case("field-64x32", 336, 208, F420, 64, 32, 2, "field", dict(seed=1, move=(1, 2), p_zero=0.25, p_move=0.8),
       ["cand.n2", "cand.dup.d2", "cand.pick.k0", "nine.k3", "bin.NB3_HD", "part.2", "win.spread_x", "win.spread_y", "win.spx_exact"])
_case("field-64x64", 384, 256, F420, 64, 64, 2, "field", dict(seed=1, move=(1, 2), p_zero=0.25, tex='smooth'),
       ["cand.n3", "cand.offgrid.L", "cand.pick.k1", "nine.k6", "body.fast.nkb16", "win.staged", "win.mis1", "nine.in_win",
        "patch.from_win.nohp"])
_case("field-64x48", 208, 148, F420, 64, 48, 2, "field", dict(seed=1, move=(0, 1, 2), p_zero=0.2),
       ["cand.n4", "cand.offgrid.R", "nine.k0", "nine.k4", "body.fast.nkb12", "win.cand_sh0", "win.cand_sh2", "patch.from_win.hp"])
_case("field-64x32-l1", 384, 256, F420, 64, 32, 1, "field", dict(seed=1, move=(1,), p_zero=0.1, steps=(-1, 1)),
       ["cand.n5", "cand.offgrid.T", "nine.k5", "nine.k7", "body.fast.nkb8", "win.zero_outside", "patch.pmis3", "nine.global"])
_case("half-64x32", 336, 208, F420, 64, 32, 2, "field", dict(seed=1, move=(1,), halfpel=True, tex='extreme'),
       ["hp.skipped", "hp.win.k2", "hp.win.k5", "hp.sat.H.hi", "hp.sat.D.hi", "clip.ref.edge_exact", "chroma.table",
        "chroma.fetch.pre"])
_case("half-64x64", 384, 256, F444, 64, 64, 1, "field", dict(seed=1, move=(0, 1), halfpel=True, tex='noise'),
       ["hp.win.k0", "hp.win.k3", "hp.win.k6", "hp.sat.V.lo", "body.fast.up.nkb16"])
_case("half-16", 125, 77, F444, 16, 16, 3, "field", dict(seed=1, move=(0, 1, 2), halfpel=True, tex='extreme'),
       ["hp.kept", "hp.win.k4", "hp.win.k7", "hp.sat.V.hi", "body.general.ragged", "chroma.fetch.dword"])
_case("cols-64x32", 320, 192, F420, 64, 32, 2, "field", dict(seed=1, move=(1,), tex='columns', halfpel=True),
       ["hp.win.k1", "hp.tie", "hp.sat.H.lo", "hp.sat.D.lo", "body.fast.up.nkb8"])
_case("field-16", 125, 77, F444, 16, 16, 3, "field", dict(seed=1, move=(0, 1, 2, 3), p_move=0.7),
       ["cand.n6", "cand.dup.d4", "cand.pick.k5", "nine.k8", "part.0", "nine.gmis3"])
_case("field-24", 101, 75, F422, 24, 24, 2, "field", dict(seed=1, move=(0, 1, 2)),
       ["cand.dup.d1", "cand.pick.k3", "nine.k2", "nine.tie", "patch.pmis1", "patch.loaded.nohp"])
_case("field-32", 162, 98, F444, 32, 32, 3, "field", dict(seed=3, move=(0, 1, 2, 3), canvas=True),
       ["cand.pick.k2", "cand.pick.k4", "nine.k1", "nine.gmis1", "patch.loaded.hp"])
_case("field-48", 150, 110, F420, 48, 48, 2, "field", dict(seed=1, move=(0, 1, 2)),
       ["cand.zero_parent", "body.general.cmask.partial", "patch.pmis0", "patch.pmis2"])
_case("clamp-neg", 44, 44, F444, 16, 16, 5, "field", dict(seed=1, move=(2, 3, 4, 5), const=(-1, -1), canvas=True, tex='smooth'),
       ["start.clamp.xlo", "start.clamp.ylo", "nine.gmis0"])
_case("clamp-pos", 44, 44, F444, 16, 16, 5, "field", dict(seed=1, move=(2, 3, 4, 5), const=(1, 1), canvas=True, tex='smooth'),
       ["start.clamp.xhi", "start.clamp.yhi", "nine.gmis2"])
_case("outside", 125, 77, F444, 16, 16, 3, "field", dict(seed=2, move=(0, 1, 2)),
       ["blk.odd_area", "blk.outside"], dims={1: (40, 30)})
_case("mix-16", 384, 256, F420, 16, 16, 1, "mix", dict(seed=1),
       ["var.chroma.nowrap", "bin.NB1_PLAIN", "bin.NB3_PLAIN", "bin.INTRA_FLATSRC", "bin.SUBMASK4", "bin.SUBMASK5", "bin.SUBMASK11",
        "bin.SUBMASK13", "bin.SUBMASK14"])
_case("mix-64x32", 336, 208, F420, 64, 32, 2, "mix", dict(seed=1),
       ["var.zero.wrap", "bin.NB0_HD", "bin.INTRA_CHROMA", "bin.SUBMASK6", "bin.SUBMASK10"])
_case("mix-64x64", 384, 256, F444, 64, 64, 1, "mix", dict(seed=1),
       ["var.chroma.wrap", "bin.NB1_HD", "bin.VETO_NOT_TAKEN", "bin.SUBMASK1", "chroma.fetch.loop"])
_case("mix-64x48", 208, 148, F420, 64, 48, 2, "mix", dict(seed=1),
       ["var.div.odd_exact", "bin.INTRA_REFVAR", "bin.INTRA_BADSAD", "bin.SUBMASK15", "body.fast.up.nkb12", "clip.src.ring"])
_case("mix-49", 305, 208, F420, 64, 32, 2, "mix", dict(seed=1),
       ["var.div.needs_bias", "bin.NB2_HD", "bin.LOWTEX_ALL_INTRA", "bin.SUBMASK3", "bin.SUBMASK12"])
_case("mix-7", 119, 71, F444, 16, 16, 2, "mix", dict(seed=1),
       ["bin.HP_REFINED", "bin.INTRA_ZEROVAR", "bin.QUAD_VOTE", "bin.SUBMASK8"])
_case("mix-24-411", 101, 75, F411, 24, 24, 2, "mix", dict(seed=1),
       ["bin.NB2_PLAIN", "bin.SUBMASK0", "bin.SUBMASK7", "bin.SUBMASK9"])
_case("mix-48", 150, 110, F420, 48, 48, 2, "mix", dict(seed=1),
       ["bin.SUBMASK2"])
_case("bias-49", 305, 208, F420, 64, 32, 2, "bias", dict(seed=0),
       ["var.div.needs_bias", "var.div.odd_exact", "bin.INTRA_NONE"])
_case("bias-7", 119, 71, F444, 16, 16, 2, "bias", dict(seed=1),
       ["var.div.needs_bias", "bin.INTRA_NONE"])
