"""The path every block of a motion search takes through `hme_block` (csrc/k_hme.hip), computed from the geometry and from the oracle's
per-block trace (oracle/orc.h: orc_hme_trace).  No GPU, nothing of the product runs.

What is RIGHT is decided by the oracle (oracle/orc_hme.c, pinned to the reference).  This module restates which CODE a block reaches --
the body, the union window, the patch, the clip and chroma arrangements -- from the facts the kernel branches on, so that the tests can
name the branch a built case is there for (tests/hme_cases.py), prove on the CPU that it is reached (test_hme_cases_host.py) and say on a
device mismatch which lines the block went through (explain, test_gpu_hme_paths.py).

The numbers the kernel branches on are read from its source, never retyped: UW_P / UW_SPX / UW_SPY / WIN (k_hme.hip), DSVG_BORDER, the
deep_r and ring rules (dsvg_kernels.hpp: hme_deep_r, hme_ring_x16, hme_ring_y4) and the block sizes of the full-block body
(hme_level_plan).  LABELS names, for every label, the line of k_hme.hip (plain numbers) or of the reference's hme.c it stands for."""
import ctypes as C
import os
import re

import numpy as np

import _cabi as A

CSRC = os.path.join(A.PKG_DIR, "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _defines(src, names):
    """#define NAME expr of `names`, evaluated in order (an expression may use an earlier name)"""
    out = {}
    for n in names:
        m = re.search(r"^#define %s\s+(.+?)\s*(?://.*)?$" % n, src, re.M)
        assert m, "k_hme.hip no longer defines %s" % n
        expr = m.group(1)
        assert re.fullmatch(r"[\w\s()+\-*/]+", expr), (n, expr)
        out[n] = int(eval(expr, {"__builtins__": {}}, dict(out)))
    return out


def _inline_rule(src, name, args):
    """the return expression of `static inline int name(args) { return expr; }` as a Python function"""
    m = re.search(r"static inline int %s\(([^)]*)\)\s*\{\s*return\s+([^;]+);" % name, src)
    assert m, "dsvg_kernels.hpp no longer has %s" % name
    got = [a.split()[-1] for a in m.group(1).split(",")]
    assert got == list(args), (name, got)
    expr = m.group(2).replace("/", "//")
    assert re.fullmatch(r"[\w\s()+\-*/<]+", expr), (name, expr)
    return lambda *v: int(eval(expr, {"__builtins__": {}}, dict(zip(args, v))))


_HME = _read("k_hme.hip")
_KRN = _read("dsvg_kernels.hpp")
_D = _defines(_HME, ["WIN", "UW_P", "UW_SPX", "UW_SPY", "HME_UNION", "HME_UNION_UPPER", "HME_PG", "HME_WPG"])
WIN, UW_SPX, UW_SPY = _D["WIN"], _D["UW_SPX"], _D["UW_SPY"]
assert _D["HME_UNION"] == 1 and _D["HME_UNION_UPPER"] == 0, "the model knows the union window on level 0 only"
BORDER = _defines(_KRN, ["DSVG_BORDER"])["DSVG_BORDER"]
deep_r = _inline_rule(_KRN, "hme_deep_r", ["levels"])
ring_x16 = _inline_rule(_KRN, "hme_ring_x16", ["blk_w", "deep_r"])
ring_y4 = _inline_rule(_KRN, "hme_ring_y4", ["blk_h", "deep_r"])
_m = re.search(r"P\.nkbf = \(([^;]+)\) \? A\.blk_h / 4 : 0;", _HME)
assert _m, "hme_level_plan's NKBF rule moved"
FAST_BW = [int(v) for v in re.findall(r"A\.blk_w == (\d+)", _m.group(1))]
FAST_BH = [int(v) for v in re.findall(r"A\.blk_h == (\d+)", _m.group(1))]
assert FAST_BW == [64] and FAST_BH and "stride[0] & 3" in _m.group(1)

HME_TABLE, HME_IN_CLIP = 1, 2                        # DSVG_HME_TABLE, DSVG_HME_IN_CLIP (include/dsvg.h)
FP = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (-1, -1), (1, -1), (-1, 1), (1, 1)]          # FP_X, FP_Y (:257-258)
HP = [(1, 0), (-1, 0), (0, 1), (0, -1), (-1, -1), (1, -1), (-1, 1), (1, 1)]                  # HP_X, HP_Y (:259-260)
COV = (["HP_SKIPPED", "HP_KEPT_FULLPEL", "HP_REFINED",
        "NB0_PLAIN", "NB1_PLAIN", "NB2_PLAIN", "NB3_PLAIN", "NB0_HD", "NB1_HD", "NB2_HD", "NB3_HD",
        "INTRA_ZEROVAR", "INTRA_REFVAR", "INTRA_FLATSRC", "INTRA_AVG", "INTRA_BADSAD", "INTRA_CHROMA", "INTRA_NONE",
        "VETO_TAKEN", "VETO_NOT_TAKEN", "LOWTEX_ALL_INTRA", "QUAD_VOTE"] + ["SUBMASK%d" % i for i in range(16)]
       + ["LO_TEX", "LO_VAR", "LO_NEITHER"])         # ORC_COV_* (oracle/orc.h) up to the level-0 block decisions: the first 38 are hme.c:544-721's
N_BINS = 38

TRACE_DTYPE = np.dtype([("visited", "<i4"), ("level", "<i4"), ("i", "<i4"), ("j", "<i4"), ("bx", "<i4"), ("by", "<i4"), ("bw", "<i4"), ("bh", "<i4"),
                        ("par", "<i4", (5,)), ("par_on", "<i4", (5,)), ("n", "<i4"), ("cand", "<i4", (6,)), ("src_ok", "<i4"), ("valid", "<i4"),
                        ("cand_sad", "<i4", (6,)), ("pick", "<i4"), ("sx", "<i4"), ("sy", "<i4"), ("cx", "<i4"), ("cy", "<i4"),
                        ("nine", "<i4", (9,)), ("nine_k", "<i4"), ("best", "<i4"), ("did_hp", "<i4"), ("hp_thr", "<i4"), ("hp", "<i4", (8,)),
                        ("hp_k", "<i4"), ("sat", "<i4", (6,)), ("wrap", "<i4", (3,)), ("src_var_neg", "<i4"), ("cov_lo", "<u4"), ("cov_hi", "<u4"),
                        ("mvx", "<i4"), ("mvy", "<i4"), ("rsv", "<i4", (6,))])
assert TRACE_DTYPE.itemsize == 80 * 4                # orc_hme_trace

LABELS = {}


def _L(name, where):
    LABELS[name] = where


for _k in range(1, 7):
    _L("cand.n%d" % _k, "456-457: %d candidate(s) after de-duplication (hme.c:452-480)" % _k)
for _k in range(1, 5):
    _L("cand.dup.d%d" % _k, "454-456: a parent equal to the one %d place(s) before it and to no other earlier one -- only the row_shr:%d compare drops it" % (_k, _k))
_L("cand.zero_parent", "456: a parent on the grid whose vector is zero (par_l != 0)")
for _k, _m2 in zip("LRTB", (1, 2, 3, 4)):
    _L("cand.offgrid." + _k, "369 / 447-450: parent %d lies outside the block grid and counts as the zero vector" % _m2)
_L("cand.invalid.src", "498: the source block fails frame_invalid")
_L("cand.invalid.ref", "508 / 584: a candidate's reference block fails frame_invalid and is not scored (hme.c:487-494)")
_L("cand.none_valid", "481,659: no candidate valid, the last one is taken unscored (pick = n - 1)")
for _k in range(6):
    _L("cand.pick.k%d" % _k, "652-659: candidate %d of several wins (hme.c:503-506)" % _k)
_L("cand.tie", "652-659: the smallest SAD is shared: the lower index wins through the (score << 3 | index) key")
_L("cand.sadmax", "656: a candidate's SAD is the largest there is, 255 * 64 * 64 = 1 044 480: acc << 3 stays below 2^23")
for _k in ("xlo", "xhi", "ylo", "yhi"):
    _L("start.clamp." + _k, "675-676: the start vector is clamped on this side (hme.c:512-517)")
for _k in range(9):
    _L("nine.k%d" % _k, "835-838: point %d of the nine wins (hme.c:519-541)" % _k)
_L("nine.tie", "835-838: the smallest of the nine SADs is shared: the first in FP order wins")
_L("hp.skipped", "874: best <= BW * BH, no half-pel search (hme.c:551)")
_L("hp.kept", "1031-1034: searched, kept full-pel: rows / columns 2..15 of the staged patch are the window")
for _k in range(8):
    _L("hp.win.k%d" % _k, "1013-1024: half-pel candidate %d wins: its own (plane, row, column) extraction" % _k)
_L("hp.tie", "1013-1014: the winning half-pel SAD is shared: the first in HP order wins")
for _p, _ln in (("H", "950"), ("V", "970-972"), ("D", "984")):
    _L("hp.sat.%s.lo" % _p, "%s: a compared %s sample is clipped at 0" % (_ln, _p))
    _L("hp.sat.%s.hi" % _p, "%s: a compared %s sample is clipped at 255" % (_ln, _p))
for _k, _ln in (("luma", "1105"), ("zero", "1107"), ("chroma", "1244-1245")):
    _L("var.%s.wrap" % _k, "%s: sum * sum passes 2^32 (hme.c:213-300: unsigned wrap)" % _ln)
    _L("var.%s.nowrap" % _k, "%s: sum * sum stays below 2^32" % _ln)
_L("var.src_var.neg", "1110: the window's variance is negative as an int (hme.c:181-211)")
_L("var.div.odd_exact", "246: udiv_rd divides a multiple of an area that is no power of two")
_L("var.div.needs_bias", "246-248: the rounded product n * (1 / d) lies below the exact integer quotient: only the 2^-16 bias makes the truncation right")
for _k in range(N_BINS):
    _L("bin." + COV[_k], "hme.c:544-721: ORC_COV_%s (oracle/orc.h)" % COV[_k])
_L("blk.full", "320: bw == BW and bh == BH")
_L("blk.partial.right", "320: bw < BW, bh == BH")
_L("blk.partial.bottom", "320: bw == BW, bh < BH")
_L("blk.partial.corner", "320: bw < BW, bh < BH")
_L("blk.narrow", "336,870,890: a level-0 block narrower or shorter than the 14x14 statistics window")
_L("blk.odd_area", "869: a level-0 block whose area is odd")
_L("blk.outside", "1377-1383: a block of the grid that starts outside the level's picture: the zero vector (hme.c:441-444)")
for _k in FAST_BH:
    _L("body.fast.nkb%d" % (_k // 4), "1556-1558: level 0, hme_block<true, %d>: the union-window body" % (_k // 4))
    _L("body.fast.up.nkb%d" % (_k // 4), "1553-1555,1386: an upper level's full block, hme_block<false, %d>" % (_k // 4))
_L("body.general.uni", "349,645,832: generic body, bh % 4 == 0: score / nine(std::true_type)")
_L("body.general.ragged", "349,645,832: generic body, bh % 4 != 0: score / nine(std::false_type), per-lane row selects")
_L("body.general.cmask.partial", "357: a lane's dword straddles the block's right edge")
_L("body.general.cmask.empty", "357: lanes whose columns lie right of the block")
for _k in range(4):
    _L("part.%d" % _k, "1339-1391,1529-1532: the block is done by a PART %d launch" % _k)
_L("win.staged", "514,519-574: the union window is staged and the candidates scored from it")
_L("win.none_valid", "514,517: no non-zero candidate is valid")
_L("win.spread_x", "514: the valid candidates are spread wider than UW_SPX")
_L("win.spread_y", "514: the valid candidates are spread higher than UW_SPY")
_L("win.spx_exact", "514: spread exactly UW_SPX, staged")
_L("win.spy_exact", "514,524: spread exactly UW_SPY, staged: UW_ROWS rows")
_L("win.zero_outside", "714: the zero vector wins from outside the candidates' box")
for _k in range(4):
    _L("win.mis%d" % _k, "522: the window's first byte sits at byte %d of its dword" % _k)
    _L("win.cand_sh%d" % _k, "557-558: a candidate's rows sit at byte %d of the staged dwords" % _k)
    _L("nine.gmis%d" % _k, "722 / 788: the nine-point window read from memory, misaligned by %d" % _k)
    _L("patch.pmis%d" % _k, "896,909 / 911-912: the patch's first pixel at byte %d" % _k)
_L("nine.in_win", "717-719: the nine-point search reads the union window")
_L("nine.global", "720-779: a full level-0 block's nine-point search reads memory")
for _a in ("from_win", "loaded"):
    for _b in ("hp", "nohp"):
        _L("patch.%s.%s" % (_a, _b), "%s: the %s, %s" % ("891-909" if _a == "from_win" else "911-912", "19x20 patch" if _b == "hp" else "14x14 window",
                                                         "taken out of the union window" if _a == "from_win" else "loaded from memory"))
_L("clip.src.clip", "337: the source rows come from the packed clip")
_L("clip.src.ring", "334-337: the statistics window leaves the picture: the source rows come from the bordered copy")
_L("clip.ref.clip", "338: deep_r or more from every edge: the reference rows come from the packed clip")
_L("clip.ref.ring", "338: nearer an edge: the reference rows come from the bordered copy's ring")
_L("clip.ref.edge_exact", "338: bx + bw + R == fw, by + bh + R == fh, bx == R or by == R: the last block that reads the clip")
_L("clip.ref.edge_short", "338: bx + bw + R == fw + 1 (or the same in y): the first block that does not")
_L("chroma.table", "1145-1152: the chroma sums come from k_hme_csum's table")
_L("chroma.fetch.pre", "1154-1196: a full block fetches its chroma blocks in whole passes")
_L("chroma.fetch.dword", "1198-1223: one aligned dword per item")
_L("chroma.fetch.loop", "1225-1239: the unaligned loop")

# Labels no input reaches.  Each entry: (why, a function of the constants that must hold -- test_hme_cases_host.py calls it).
UNREACHABLE = {
    "cand.invalid.src": ("320,498: bx < fw and bw = min(fw - bx, BW) (a full block: 64 <= fw - bx): the source block never leaves the picture, let alone the border",
                         lambda: BORDER >= 0),
    "cand.none_valid": ("508: the zero vector's reference block is the source block's own place, valid whenever the source is (above)", lambda: BORDER >= 0),
    "win.none_valid": ("514: a full block's candidate is valid unless it leaves the border, i.e. is longer than the border: a level-0 start vector is at "
                       "most 2^(levels+1) - 2 <= 62 pixels long", lambda: (2 << 5) - 2 < BORDER),
    "win.mis0": ("522: a level-0 candidate is a level-1 vector, dx << 1 (:843), hence even, and a full block's bx is a multiple of 64: bx + xmn - 1 is odd",
                 lambda: all(b % 4 == 0 for b in FAST_BW)),
    "win.mis2": ("522: as win.mis0", lambda: all(b % 4 == 0 for b in FAST_BW)),
    "win.cand_sh1": ("557-558: cdx - xmn is even (as win.mis0) and 1 + wmis is even", lambda: all(b % 4 == 0 for b in FAST_BW)),
    "win.cand_sh3": ("557-558: as win.cand_sh1", lambda: all(b % 4 == 0 for b in FAST_BW)),
    "var.src_var.neg": ("1110: the sum of a 14x14 window is below 2^16, so its square does not wrap; sum of squares - floor(sum^2 / 196) is then at least "
                        "the window's variance times 196, never negative, and below 2^31", lambda: WIN * WIN * 255 < 1 << 16 and WIN * WIN * 255 * 255 < 1 << 31),
    "clip.ref.edge_short": ("338: R is even for every level count, luma in place needs w % 16 == 0 and h % 4 == 0 and full-size blocks are even: "
                            "bx + bw + R is even, fw + 1 odd", lambda: all(deep_r(l) % 2 == 0 for l in range(6))),
    "cand.invalid.ref": ("508,584: a start vector is at most 2^(levels+1) - 2 <= 62 pixels long (a level adds +-1 of its own pixels to twice its parent's vector, "
                         "hme.c:452-541) and the block lies inside the picture: its displaced copy stays inside the border.  frame_invalid can only fire "
                         "on fields the search did not make itself", lambda: (2 << 5) - 2 < BORDER),
}
# Labels whose only known route is a picture wider than 4096 pixels stay with fwd_cases.py's 4160-wide cases (test_gpu_fwd_paths.py):
# k_hme_csum declining for fullx > 64 (csum "early-out", k_hme.hip:1410,1473), the search then fetching with a table allocated.
ELSEWHERE = ("csum.early-out",)


def rsu(x, s):
    return (x + (1 << s) - 1) >> s


class Geo:
    """a picture, its block grid, its pyramid and the launches hme_plan (k_hme.hip:1495-1537) makes for it"""

    def __init__(self, w, h, fmt, bw, bh, levels, dims=None):
        """dims: {level: (w, h)} of upper-level pictures that are not the halvings of the one below (the operator takes every level's frames as
        they come): smaller ones leave blocks of the grid outside the picture"""
        self.w, self.h, self.fmt, self.bw, self.bh, self.levels = w, h, fmt, bw, bh, levels
        self.nxb, self.nyb = -(-w // bw), -(-h // bh)
        self.nblk = self.nxb * self.nyb
        self.hs, self.vs = A.hshift(fmt), A.vshift(fmt)
        self.dims = [(dims or {}).get(l, (rsu(w, l), rsu(h, l))) for l in range(levels + 1)]
        self.name = "%dx%d-%s-b%dx%d-l%d" % (w, h, {0: "444", 4: "422", 5: "420", 8: "411"}[fmt], bw, bh, levels)
        self.R = deep_r(levels)
        self.in_clip_ok = w % 16 == 0 and h % 4 == 0                             # dsvg_op_hme_ex (dsvg_ops.hip)
        self.ring = (16 * ring_x16(bw, self.R), 4 * ring_y4(bh, self.R))

    def level_plan(self, l):
        """hme_level_plan (k_hme.hip:1476-1491): (nkbf, fullx, fully, parts mask)"""
        step = 1 << l
        nvx, nvy = (self.nxb + step - 1) // step, (self.nyb + step - 1) // step
        fw, fh = self.dims[l]
        stride = (fw + 2 * BORDER + 15) & ~15
        nkbf = self.bh // 4 if self.bw in FAST_BW and self.bh in FAST_BH and stride % 4 == 0 else 0
        fullx, fully = (min(nvx, fw // 64), min(nvy, fh // self.bh)) if nkbf else (0, 0)
        nfull = fullx * fully
        if nfull and l:
            parts = 1 << 3
        elif nfull:
            parts = 1 << 1 | (1 << 2 if nvx * nvy - nfull else 0)
        else:
            parts = 1
        return nkbf, fullx, fully, parts

    def csum(self, flags):
        """hme_csum_plan (k_hme.hip:1468-1474)"""
        if not flags & HME_TABLE:
            return 0
        nkbf, fullx, fully, _ = self.level_plan(0)
        if not (fullx and fully):
            return 0
        return 2 if ((self.bw >> self.hs) & 15) or fullx > 64 else 1

    def dispatch(self, flags):
        """what dsvg_dispatch_last reports after the search: ([per level (nkbf, fullx, fully, parts)], csum)"""
        return [self.level_plan(l) for l in range(self.levels + 1)], self.csum(flags)

    def has_fast0(self):
        nkbf, fullx, fully, _ = self.level_plan(0)
        return bool(nkbf and fullx and fully)


def _s16(v):
    return ((v & 0xffff) ^ 0x8000) - 0x8000


def vec(all_, level):
    """(x, y) of a packed vector in the pixels of `level` (arithmetic shifts, as :507)"""
    return _s16(all_) >> level, _s16(all_ >> 16) >> level


def _needs_bias(n, d):
    return int(float(n) * (1.0 / d)) != n // d


def block_labels(geo, t, flags=0):
    """the labels of one traced block; `t` is a record of TRACE_DTYPE, flags the operator's (clip.* and chroma.table exist only with them)"""
    out = set()
    l = int(t["level"])
    if t["visited"] == 2:
        return {"blk.outside", "part.%d" % _part(geo, t)}
    bx, by, bw, bh = int(t["bx"]), int(t["by"]), int(t["bw"]), int(t["bh"])
    fw, fh = geo.dims[l]
    nkbf = geo.level_plan(l)[0]
    fast = bool(nkbf) and fw - bx >= 64 and fh - by >= geo.bh                    # :1386; PART 1: i < fullx, j < fully is the same thing
    out.add("part.%d" % _part(geo, t))
    out.add("blk.full" if (bw, bh) == (geo.bw, geo.bh) else "blk.partial." + ("corner" if bw < geo.bw and bh < geo.bh else "right" if bw < geo.bw else "bottom"))
    if fast:
        out.add("body.fast.%snkb%d" % ("up." if l else "", nkbf))
    else:
        out.add("body.general.uni" if bh % 4 == 0 else "body.general.ragged")
        if bw % 4:
            out.add("body.general.cmask.partial")
        if bw < 64 - 3:
            out.add("body.general.cmask.empty")
    # ---- candidates (:402-465)
    n = int(t["n"])
    out.add("cand.n%d" % n)
    par = [int(v) for v in t["par"]]
    on = [int(v) for v in t["par_on"]]
    if l < geo.levels:
        for m in range(5):
            if not on[m]:
                out.add("cand.offgrid." + "?LRTB"[m])
            elif par[m] == 0:
                out.add("cand.zero_parent")
            else:
                same = [k for k in range(1, m + 1) if par[m - k] == par[m]]
                if len(same) == 1:
                    out.add("cand.dup.d%d" % same[0])
    cands = [vec(int(t["cand"][k]), l) for k in range(n)]
    valid = int(t["valid"])
    if n > 1:
        if not t["src_ok"]:
            out.add("cand.invalid.src")
        elif valid != (1 << n) - 1:
            out.add("cand.invalid.ref")
        if valid == 0:
            out.add("cand.none_valid")
        else:
            out.add("cand.pick.k%d" % int(t["pick"]))
            sads = [int(t["cand_sad"][k]) for k in range(n) if valid >> k & 1]
            if sads.count(min(sads)) > 1:
                out.add("cand.tie")
            if max(sads) == 255 * 64 * 64:
                out.add("cand.sadmax")
    sx, sy, cx, cy = (int(t[k]) for k in ("sx", "sy", "cx", "cy"))
    if cx > sx:
        out.add("start.clamp.xlo")
    if cx < sx:
        out.add("start.clamp.xhi")
    if cy > sy:
        out.add("start.clamp.ylo")
    if cy < sy:
        out.add("start.clamp.yhi")
    nine = [int(v) for v in t["nine"]]
    out.add("nine.k%d" % int(t["nine_k"]))
    if nine.count(min(nine)) > 1:
        out.add("nine.tie")
    mvx, mvy = cx + FP[int(t["nine_k"])][0], cy + FP[int(t["nine_k"])][1]        # the full-pel vector
    if l:
        if not fast:
            out.add("nine.gmis%d" % ((bx + cx - 1) & 3))
        return out
    # ---- level 0
    if bw < WIN or bh < WIN:
        out.add("blk.narrow")
    if (bw * bh) & 1:
        out.add("blk.odd_area")
    have_win = False
    if fast:
        nz = [cands[k] for k in range(1, n) if valid >> k & 1]
        if n > 1:
            if not nz:
                out.add("win.none_valid")
            else:
                xs, ys = [c[0] for c in nz], [c[1] for c in nz]
                xmn, xmx, ymn, ymx = min(xs), max(xs), min(ys), max(ys)
                if xmx - xmn > UW_SPX:
                    out.add("win.spread_x")
                if ymx - ymn > UW_SPY:
                    out.add("win.spread_y")
                have_win = xmx - xmn <= UW_SPX and ymx - ymn <= UW_SPY
                if have_win:
                    out.add("win.staged")
                    if xmx - xmn == UW_SPX:
                        out.add("win.spx_exact")
                    if ymx - ymn == UW_SPY:
                        out.add("win.spy_exact")
                    wmis = (bx + xmn - 1) & 3                                    # :522 (strides, offsets and slabs are multiples of 4)
                    out.add("win.mis%d" % wmis)
                    for c in nz:
                        out.add("win.cand_sh%d" % ((c[0] - xmn + 1 + wmis) & 3))
                    if not (xmn <= cx <= xmx and ymn <= cy <= ymx):
                        out.add("win.zero_outside")
                        have_win = False
        out.add("nine.in_win" if have_win else "nine.global")
    if not have_win:
        out.add("nine.gmis%d" % ((bx + cx - 1) & 3))
    did_hp = bool(t["did_hp"])
    e = 2 if did_hp else 0
    wx = bx + (bw >> 1) - WIN // 2
    if have_win:
        out.add("patch.from_win." + ("hp" if did_hp else "nohp"))
        out.add("patch.pmis%d" % (((bw >> 1) - WIN // 2 + mvx - e - (xmn - 1) + wmis) & 3))
    else:
        out.add("patch.loaded." + ("hp" if did_hp else "nohp"))
        out.add("patch.pmis%d" % ((wx + mvx - e) & 3))
    if not did_hp:
        out.add("hp.skipped")
    else:
        hk = int(t["hp_k"])
        out.add("hp.kept" if hk < 0 else "hp.win.k%d" % hk)
        hp = [int(v) for v in t["hp"]]
        if hk >= 0 and hp.count(hp[hk]) > 1:
            out.add("hp.tie")
        for q, nm in enumerate(("H.lo", "H.hi", "V.lo", "V.hi", "D.lo", "D.hi")):
            if t["sat"][q]:
                out.add("hp.sat." + nm)
    out.add("var.luma." + ("wrap" if t["wrap"][0] else "nowrap"))
    out.add("var.zero." + ("wrap" if t["wrap"][1] else "nowrap"))
    if t["wrap"][2] >= 0:
        out.add("var.chroma." + ("wrap" if t["wrap"][2] else "nowrap"))
    if t["src_var_neg"]:
        out.add("var.src_var.neg")
    cov = int(t["cov_lo"]) | int(t["cov_hi"]) << 32
    for b in range(N_BINS):
        if cov >> b & 1:
            out.add("bin." + COV[b])
    # ---- luma in place (:330-339)
    if flags & HME_IN_CLIP:
        R = geo.R
        wy = by + (bh >> 1) - WIN // 2
        out.add("clip.src.clip" if wx >= 0 and wy >= 0 and wx + WIN <= fw and wy + WIN <= fh else "clip.src.ring")
        deep = bx >= R and by >= R and bx + bw + R <= fw and by + bh + R <= fh
        out.add("clip.ref.clip" if deep else "clip.ref.ring")
        if deep and (bx + bw + R == fw or by + bh + R == fh or bx == R or by == R):
            out.add("clip.ref.edge_exact")
        if not deep and (bx + bw + R == fw + 1 or by + bh + R == fh + 1):
            out.add("clip.ref.edge_short")
    # ---- the chroma variance test (:1129-1248)
    if t["wrap"][2] >= 0:
        cbw, cbh = bw >> geo.hs, bh >> geo.vs
        cbx = int(t["i"]) * (geo.bw >> geo.hs)
        ndw = (cbw + 3) >> 2
        if fast and flags & HME_TABLE and cbw % 16 == 0 and geo.nxb <= 64:
            out.add("chroma.table")
        elif fast and cbx % 4 == 0 and cbw % 4 == 0 and ndw >= 4 and ndw & (ndw - 1) == 0 and ndw <= 16 and cbh % (64 // ndw) == 0 and cbh // (64 // ndw) <= 4:
            out.add("chroma.fetch.pre")
        elif cbx % 4 == 0 and ndw * cbh <= 256:
            out.add("chroma.fetch.dword")
        else:
            out.add("chroma.fetch.loop")
    return out


def _part(geo, t):
    l = int(t["level"])
    nkbf, fullx, fully, parts = geo.level_plan(l)
    if parts & 8:
        return 3
    if parts & 1:
        return 0
    step = 1 << l
    return 1 if int(t["i"]) // step < fullx and int(t["j"]) // step < fully else 2


def div_labels(geo, src_y, ref_y, t):
    """var.div.*: the divisions udiv_rd (:246) does for a level-0 block on sums that the pixels alone decide: the block's and the
    zero-motion block's sum * sum mod 2^32, the gradient sum and the zero-motion sum, each by the block's area"""
    bx, by, bw, bh = int(t["bx"]), int(t["by"]), int(t["bw"]), int(t["bh"])
    area = bw * bh
    out = set()
    if area & (area - 1) == 0:
        return out
    for pl in (src_y, ref_y):
        b = pl[by:by + bh, bx:bx + bw].astype(np.int64)
        s1 = int(b.sum())
        for n in ((s1 * s1) & 0xffffffff, s1):
            if n and n % area == 0:
                out.add("var.div.odd_exact")
                if _needs_bias(n, area):
                    out.add("var.div.needs_bias")
    return out


def run_oracle(orc, geo, src, ref):
    """the oracle's search of one pair with its trace: (intra %, [field of level l as MV_DTYPE], trace as TRACE_DTYPE[levels + 1][nblk])"""
    meta = A.Meta(geo.w, geo.h, geo.fmt, 30, 1, 1, 1)
    prm = A.Params(C.pointer(meta), 1, 1, geo.bw, geo.bh, geo.nxb, geo.nyb)
    hm = A.HME()
    hm.params = C.pointer(prm)
    hm.levels = geo.levels
    for l in range(geo.levels + 1):
        hm.src[l] = C.pointer(src[l].c)
        hm.ref[l] = C.pointer(ref[l].c)
    tr = np.zeros((geo.levels + 1, geo.nblk), dtype=TRACE_DTYPE)
    orc.orc_hme_run_trace.restype = C.c_int
    orc.orc_hme_run_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    pct = orc.orc_hme_run_trace(C.addressof(hm), tr.ctypes.data, tr.size)
    fields = []
    for l in range(geo.levels + 1):
        fields.append(np.ctypeslib.as_array(C.cast(hm.mvf[l], C.POINTER(C.c_uint8)), shape=(geo.nblk * 12,)).copy().view(A.MV_DTYPE))
        C.CDLL(None).free(hm.mvf[l])
    return pct, fields, tr


def labels_of(geo, tr, src, ref, flags=0):
    """{(level, block index): labels} of a traced search; src / ref: the pair's level frames (BorderedFrame); flags: the operator's,
    or a list of them: the union over the calls"""
    if isinstance(flags, (list, tuple)):
        out = {}
        for f in flags:
            for k, v in labels_of(geo, tr, src, ref, f).items():
                out.setdefault(k, set()).update(v)
        return out
    out = {}
    sy, ry = src[0].plane(0), ref[0].plane(0)
    for l in range(geo.levels + 1):
        for b in range(geo.nblk):
            t = tr[l, b]
            if not t["visited"]:
                continue
            s = block_labels(geo, t, flags)
            if l == 0 and t["visited"] == 1:
                s |= div_labels(geo, sy, ry, t)
            out[(l, b)] = s
    return out


def reads(geo, t):
    """the luma rectangles (x0, y0, x1, y1: exclusive ends, in the level's picture) the reference's code reads for one traced block:
    [(frame 'src' / 'ref', rect)] -- the scored candidates, the nine points, the lattice's 19x20 patch, the windows"""
    l = int(t["level"])
    bx, by, bw, bh = int(t["bx"]), int(t["by"]), int(t["bw"]), int(t["bh"])
    out = [("src", (bx, by, bx + bw, by + bh))]
    for k in range(int(t["n"])):
        if int(t["valid"]) >> k & 1:
            dx, dy = vec(int(t["cand"][k]), l)
            out.append(("ref", (bx + dx, by + dy, bx + dx + bw, by + dy + bh)))
    cx, cy = int(t["cx"]), int(t["cy"])
    out.append(("ref", (bx + cx - 1, by + cy - 1, bx + cx + bw + 1, by + cy + bh + 1)))
    if l == 0:
        wx, wy = bx + (bw >> 1) - WIN // 2, by + (bh >> 1) - WIN // 2
        mvx, mvy = cx + FP[int(t["nine_k"])][0], cy + FP[int(t["nine_k"])][1]
        out.append(("src", (wx, wy, wx + WIN, wy + WIN)))
        if t["did_hp"]:
            out.append(("ref", (wx + mvx - 2, wy + mvy - 2, wx + mvx + 17, wy + mvy + 18)))      # build_lattice: columns -2..16, rows -2..17 of the window
        else:
            out.append(("ref", (wx + mvx, wy + mvy, wx + mvx + WIN, wy + mvy + WIN)))
        out.append(("ref", (bx, by, bx + bw, by + bh)))                                          # the zero-motion block
    return out


def explain(geo, labels, l, b, field, got, want):
    i, j = b % geo.nxb, b // geo.nxb
    return "%s level %d block (%d, %d) field %s: got %s want %s\n  the block's path: %s" % (
        geo.name, l, i, j, field, got, want, ", ".join("%s [%s]" % (k, LABELS[k].split(":")[0]) for k in sorted(labels.get((l, b), ()))))
