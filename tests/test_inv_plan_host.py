"""CPU checks of the inverse-transform matrix (tests/inv_cases.py) against the restated dispatch (tests/inv_plan.py).

The matrix must hold one case of every dispatch class the product has on the geometries it codes, so a new branch of
launch_inv_sbt fails here until a case is added; and together with the operator twin the cases must reach every inverse
kernel of DSVG_KERNEL_IDS but the ones listed as unreachable.  Whether the restatement is the product's dispatch is checked here,
on the CPU: it is compared with the launcher's own plan (dsvg_inv_plan: inv_sbt_plan, which launch_inv_sbt runs step by step; no
device needed) on every case, every geometry the sweep keeps and a sample of the sweep's domain, and the product's plan is checked
to cover every plane once in every configuration a caller can ask for.  That the kernels then ran as planned is checked on the GPU
(tests/test_gpu_inv_paths.py: launches and algorithmic bytes of every inverse kernel against the plan)."""
import ctypes as C
import functools
import importlib
import itertools
import os
import random
import re

import numpy as np
import pytest

import _cabi as A
import inv_cases as IC
import inv_plan as P

HOST_HPP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "digital-subband-video-1_amd", "csrc", "dsvg_host.hpp")


@functools.lru_cache(maxsize=None)
def swept():
    return P.sweep()


def inverse_kernel_ids():
    """every k_inv_* name of DSVG_KERNEL_IDS (dsvg_host.hpp)"""
    with open(HOST_HPP) as f:
        names = re.findall(r'X\(KID_\w+, "([^"]+)"\)', f.read())
    assert len(names) > 40, "DSVG_KERNEL_IDS not found"
    return {n for n in names if P.re_inverse.match(n)}


def test_matrix_covers_every_dispatch_class():
    want = swept()
    got = {}
    for g in IC.GEOMETRIES:
        got.setdefault(P.plan(*g).cls, []).append(g)
    missing = {P.describe(c): k[0] for c, k in want.items() if c not in got}
    assert not missing, "dispatch classes without a case (smallest geometry of each): %s" % missing
    extra = {P.describe(c): k for c, k in got.items() if c not in want}
    assert not extra, "cases of classes the sweep does not find: %s" % extra
    twice = {P.describe(c): k for c, k in got.items() if len(k) > 1}
    assert not twice, "classes with more than one case: %s" % twice


def test_matrix_takes_the_smallest_geometry_of_each_class():
    """(the oracle codes every one of them: no class needed its second-smallest geometry)"""
    want = swept()
    for g in IC.GEOMETRIES:
        assert want[P.plan(*g).cls][0] == g, (g, P.describe(P.plan(*g).cls))


def test_matrix_reaches_every_inverse_kernel():
    ids = inverse_kernel_ids()
    reached = set()
    for g in IC.GEOMETRIES:
        p = P.plan(*g)
        reached |= set(p.p_kernels) | set(p.i_kernels)
    assert not reached & set(P.UNREACHABLE), "listed as unreachable but planned: %s" % (reached & set(P.UNREACHABLE))
    assert reached | P.TWIN_KERNELS | set(P.UNREACHABLE) == ids, \
        "inverse kernels neither planned, nor the twin's, nor listed as unreachable: %s; unknown names: %s" % (
            ids - reached - P.TWIN_KERNELS - set(P.UNREACHABLE), (reached | P.TWIN_KERNELS | set(P.UNREACHABLE)) - ids)
    # the matrix reaches the symbol-path kernels, the twin the int32 ones: both are needed
    assert not reached <= P.TWIN_KERNELS and not P.TWIN_KERNELS <= reached


def strip_cells(g, tcx, tcy):
    """level-3 cells of the L-shaped strip launch from tile column tcx / tile row tcy on (inv_sbt_plan's strips step)"""
    x0, y0 = min(tcx * P.IT_TX, g.w3), min(tcy * P.IT_TY, g.h3)
    return (g.w3 - x0) * g.h3 + x0 * (g.h3 - y0)


@pytest.mark.parametrize("g", IC.GEOMETRIES, ids=IC.case_id)
def test_plan_covers_each_plane_once(g):
    """the branches of a P picture take every level-3 cell of every plane exactly once: the fast tiles or the patch kernel's
    rectangle plus the general strips; the fused border only where the patch kernel takes the chroma planes whole; one launch
    per kernel"""
    p = P.plan(*g)
    gy, gc = p.geos[0], p.geos[1]
    k = p.p_kernels
    assert all(n == 1 for n, _ in k.values()), k
    L, Ch = p.luma, p.chroma
    if L["kind"] == "fast":
        fast = min(L["fxg"] * P.IT_TX, gy.w3) * min(L["fyg"] * P.IT_TY, gy.h3)
        assert fast + strip_cells(gy, L["fxg"], L["fyg"]) == gy.w3 * gy.h3
        assert (L["nrest"] == 0) == (P.KPIX_SYM_F not in k) and P.KP_TILE_F in k
    else:
        assert set(k) & {P.KP_TILE_F, P.KPIX_SYM_F} == {P.KPIX_SYM_F}
    assert Ch["imax"] * Ch["jmax"] + strip_cells(gc, Ch["tcx"], Ch["tcy"]) == gc.w3 * gc.h3
    assert (P.KPATCH_C in k) == (Ch["imax"] * Ch["jmax"] > 0)
    assert (P.KPIX_SYM in k) == (Ch["right_strip"] or Ch["bottom_strip"])
    if Ch["part4"]:
        assert Ch["jmax"] == gc.h3 and gc.ph % 8 == 4            # the half-height last patch row stays with the patch kernel
    if Ch["fb"]:
        assert Ch["imax"] == gc.w3 and Ch["jmax"] == gc.h3 and P.KPIX_SYM not in k


@functools.lru_cache(maxsize=None)
def package():
    return importlib.import_module("digital-subband-video-1_amd")


def product_plan(w, h, fmt):
    """the encoder's configuration asked of dsvg_inv_plan, in the shape of inv_plan.Plan: (p_kernels, i_kernels, luma, chroma)"""
    pkg = package()
    G = P.plane_geos(w, h, fmt)
    k54 = (1, float(sum(g.w3 * g.h3 for g in G)) * 8.0)      # launch_inv54_all is not part of the query: the plan's own entry
    pk, ik = {P.K54_ALL: k54}, {P.K54_ALL: k54}

    def book(k, steps):
        for s in steps:
            P._add(k, s["kernel"], s["bytes"])
        return {s["kernel"]: s for s in steps}

    for group in (0, 1):                                      # I pictures: insym = 1, with_tail = 2, luma then chroma
        steps, fb = pkg.inv_plan(w, h, fmt, group, 0, with_tail=2, insym=1)
        assert not fb
        book(ik, steps)
    steps, fb = pkg.inv_plan(w, h, fmt, 0, 1, with_tail=2, insym=1, patch_kernel=1)
    assert not fb
    by = book(pk, steps)
    if P.KP_TILE_F in by:
        s, r = by[P.KP_TILE_F], by.get(P.KPIX_SYM_F)
        (fxg, fyg, _), (ec, eb) = s["grid"], s["args"][:2]
        luma = dict(kind="fast", fx=fxg if ec < 0 else ec, fy=fyg if eb < 0 else eb, er=ec >= 0, eb=eb >= 0, fxg=fxg, fyg=fyg,
                    nrest=r["grid"][0] if r else 0)
        assert (ec < 0 or ec == fxg - 1) and (eb < 0 or eb == fyg - 1)
        if r:
            assert r["args"][:2] == (fxg, -fyg - 1) and r["grid"][1] == 1
    else:
        assert list(by) == [P.KPIX_SYM_F] and by[P.KPIX_SYM_F]["args"][:2] == (0, 0)
        luma = dict(kind="general")
    steps, fb = pkg.inv_plan(w, h, fmt, 1, 1, with_tail=2, insym=1, patch_kernel=1, fuse_border=1)
    by = book(pk, steps)
    g = G[1]
    tgx, tgy = -(-g.w3 // P.IT_TX), -(-g.h3 // P.IT_TY)
    s, r = by.get(P.KPATCH_C), by.get(P.KPIX_SYM)
    assert set(by) <= {P.KPATCH_C, P.KPIX_SYM}
    imax, jmax, jpart, sfb = s["args"] if s else (0, 0, -1, 0)
    assert sfb == fb and jpart in (-1, g.h3 - 1)
    tcx, tcy = (r["args"][0], -r["args"][1] - 1) if r else (tgx, tgy)
    if not s:                         # no patch step: one of imax / jmax is 0, the other what the strips' tile column / row says
        imax, jmax = (g.w3 if tcx >= tgx else tcx * P.IT_TX), (g.h3 if tcy >= tgy else tcy * P.IT_TY)
    chroma = dict(imax=imax, jmax=jmax, part4=jpart >= 0, tcx=tcx, tcy=tcy, nrest=r["grid"][0] if r else 0, fb=bool(fb))
    return pk, ik, luma, chroma


def restated_plan(w, h, fmt):
    p = P.plan(w, h, fmt)
    L, Ch = p.luma, p.chroma
    luma = {k: L[k] for k in ("kind", "fx", "fy", "er", "eb", "fxg", "fyg", "nrest")} if L["kind"] == "fast" else dict(kind="general")
    if L["kind"] == "general":        # (fx and fy are no output of the product's plan there: only that they are not both positive)
        assert not (L["fx"] > 0 and L["fy"] > 0)
    chroma = {k: Ch[k] for k in ("imax", "jmax", "part4", "tcx", "tcy", "nrest", "fb")}
    if Ch["imax"] * Ch["jmax"] == 0:  # no patch step: part4 has no step to show in (it only moved tcy, which is compared)
        chroma["part4"] = False
    return p.p_kernels, p.i_kernels, luma, chroma


def test_plan_is_the_launchers_decision():
    """dsvg_inv_plan runs inv_sbt_plan -- the plan launch_inv_sbt executes -- on the geometry tables of an encoder context: in the
    encoder's configuration it is inv_plan.Plan in the names, launches and bytes of the kernels of a P and of an I picture and in
    the branch parameters of luma (fx, fy, er, eb, fxg, fyg, nrest) and chroma (imax, jmax, part4, tcx, tcy, nrest, fb), on every
    case, every geometry the sweep keeps and a sample of the sweep's domain in all four formats"""
    rnd = random.Random(0x1D5)
    dom = list(P.sweep_domain())
    sample = [(w, h, fmt) for w, h in rnd.sample(dom, 6000) for fmt in P.FORMATS.values()]
    kept = [g for k in swept().values() for g in k]
    for g in list(IC.GEOMETRIES) + kept + sample:
        assert product_plan(*g) == restated_plan(*g), g
    pkg = package()
    assert pkg.lib().dsvg_inv_plan(30, 32, 0, 0, 1, 2, 1, 1, 0, 0, 1, None, 0, None) < 0


def cover_rects(step, g):
    """the rectangles of level-3 cells (x0, x1, y0, y1) of plane g whose pixels a step of the product's plan writes"""
    pkg = package()
    kind, cx, cy = step.cover, step.cx, step.cy
    if kind == pkg.INV_COVER_NONE:
        return []
    if kind == pkg.INV_COVER_WHOLE:
        return [(0, g.w3, 0, g.h3)]
    if kind == pkg.INV_COVER_RECT:
        return [(0, cx, 0, cy)]
    assert kind == pkg.INV_COVER_FROM
    x0, y0 = min(cx * P.IT_TX, g.w3), min(cy * P.IT_TY, g.h3)
    return [(x0, g.w3, 0, g.h3), (0, x0, y0, g.h3)]


def test_product_plan_covers_each_plane_once():
    """on the product's own steps, in every configuration a caller can pass (isP x group x insym x patch_kernel x fuse_border, with
    the tail and the levels 5..4 of its own or without -- on the random geometries without, they write no pixels --: the encoder's, the decoder's with symbols on neither, one or both plane
    kinds, the operator twin's) without a switch and with each of the four alone: the steps that write pixels take every level-3
    cell of every plane of the group exactly once (rectangles inside the plane, disjoint, their areas the plane's); fb only where
    a patch step takes the planes whole and there is no strip step; at most one launch per kernel id"""
    pkg = package()
    L = pkg.lib()
    rnd = random.Random(0xC0E5)
    dom = list(P.sweep_domain())
    geos = list(IC.GEOMETRIES) + [(w, h, fmt) for fmt in P.FORMATS.values() for w, h in rnd.sample(dom, 500)]
    # isP, group, with_tail, insym, patch_kernel, fuse_border (patch_kernel only with insym: the flags it stands for come with the symbols)
    configs = [c for c in itertools.product((0, 1), (0, 1), (1, 2), (0, 1), (0, 1), (0, 1)) if c[3] or not c[4]]
    switches = (0, pkg.INV_NO_PATCH_PART, pkg.INV_NO_EDGE_TILES, pkg.INV_NO_FUSED_BORDER, pkg.INV_NO_XCD_ORDER)
    names = [L.dsvg_prof_kernel_name(i).decode() for i in range(L.dsvg_prof_kernels())]
    patch_c, p_tiles = names.index(P.KPATCH_C), [names.index(n) for n in (P.KP_TILE_F, P.KP_TILE)]
    steps, fb = (pkg.InvStep * 5)(), C.c_int(0)
    for w, h, fmt in geos:
        G = P.plane_geos(w, h, fmt)
        for (isP, group, wt, insym, pk, fuse), sw in itertools.product(configs, switches):
            if wt == 1 and (w, h, fmt) not in IC.GEOMETRIES:
                continue
            n = L.dsvg_inv_plan(w, h, fmt, group, isP, wt, insym, pk, fuse, sw, 3, steps, 5, C.byref(fb))
            what = (w, h, fmt, isP, group, wt, insym, pk, fuse, sw)
            assert 1 <= n <= 5, what
            S = steps[:n]
            assert len({s.kernel for s in S}) == n, what
            patch = [s for s in S if s.kernel == patch_c]
            for g in G[1:] if group else G[:1]:
                rects = [r for s in S for r in cover_rects(s, g)]
                assert all(0 <= x0 < x1 <= g.w3 and 0 <= y0 < y1 <= g.h3 for x0, x1, y0, y1 in rects if (x1 - x0) * (y1 - y0)), (what, rects)
                assert sum((x1 - x0) * (y1 - y0) for x0, x1, y0, y1 in rects) == g.w3 * g.h3, (what, rects)
                assert not any(a[0] < b[1] and b[0] < a[1] and a[2] < b[3] and b[2] < a[3] for a, b in itertools.combinations(rects, 2)), (what, rects)
                if fb.value:
                    assert len(patch) == 1 and (patch[0].cx, patch[0].cy) == (g.w3, g.h3), what
            if fb.value:
                assert isP and group == 1 and fuse and insym and pk and not sw & (pkg.INV_NO_FUSED_BORDER | pkg.INV_NO_PATCH_PART), what
                assert not any(s.cover == pkg.INV_COVER_FROM for s in S), what
            assert all(s.args[3] == fb.value for s in patch), what
            # what each switch takes away
            if sw & pkg.INV_NO_PATCH_PART:
                assert all(s.args[2] == -1 for s in patch), what
            if sw & pkg.INV_NO_EDGE_TILES:
                assert all(tuple(s.args[:2]) == (-1, -1) for s in S if s.kernel in p_tiles), what
            assert all(s.xcd in ((0, 2) if sw & pkg.INV_NO_XCD_ORDER else (0, 1)) for s in S), what


def test_coarse_content_engages_the_luma_filter(orc):
    """At the coarse content's quantiser the luma smoothing filter changes pixels: the oracle's inverse transform of a forward-
    transformed frame of that content, quantised as in test_gpu_ops.test_fwd_inv_sbt, differs between the luma (c = 0,
    filtered) and the chroma (c = 1) variant."""
    c = IC.CONTENTS["coarse"]
    q = A.orc_cfg(256, 80, IC.F444, **IC.cli("coarse")).quality        # the CRF quantiser of the content's qp
    assert q > 0
    for w, h in ((144, 80), (256, 136), (32, 32)):
        clip = IC.make_content(w, h, IC.F444, "coarse", 0x7117)
        f = A.BorderedFrame(w, h, IC.F444)
        f.load_planar(clip[1])
        orc.orc_frame_extend(f.ptr())
        co = np.zeros(w * h, dtype=np.int32)
        orc.orc_fwd_sbt(C.byref(f.c.planes[0]), C.byref(A.Coefs(A.i32p(co), w, h)), 1)
        co[1:] = (co[1:] // 24) * 24
        out = []
        for cc in (0, 1):
            a = co.copy()
            fo = A.BorderedFrame(w, h, IC.F444)
            orc.orc_inv_sbt(C.byref(fo.c.planes[cc]), C.byref(A.Coefs(A.i32p(a), w, h)), q, 1, cc)
            out.append(fo.plane(cc).copy())
        assert np.count_nonzero(out[0] != out[1]) > 0, "style %d at q %d: the filter left %dx%d unchanged" % (c["style"], q, w, h)
