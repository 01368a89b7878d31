"""CPU checks of the forward / motion-search matrix (tests/fwd_cases.py) against the restated dispatch (tests/fwd_plan.py).

The matrix must hold one case of every value of every axis the sweep finds, each the smallest geometry of its value that the
oracle codes, so a new branch of launch_fwd_sbt or launch_hme fails here until a case is added.  The restatement is compared with
the launchers' own decision functions (dsvg_dispatch_plan: no device needed) and with the plans they execute step by step
(dsvg_fwd_plan, dsvg_hme_plan: kernels, launches, bytes, grids, strides, counts) on every case and on a sample of the sweep; that
the kernels then ran as planned is checked on the GPU (tests/test_gpu_fwd_paths.py).  The contents must do on the oracle's streams
what they are there for."""
import ctypes as C
import functools
import importlib
import random
import subprocess
import sys

import pytest

import _cabi as A
import fwd_cases as FC
import fwd_plan as P


@functools.lru_cache(maxsize=None)
def swept():
    return P.sweep()


def case_values():
    got = {}
    for g in FC.GEOMETRIES:
        for ax, v in P.plan(*g).axes().items():
            got.setdefault((ax, v), []).append(g)
    return got


def test_matrix_names_every_axis_value_and_no_other():
    want, got = swept(), case_values()
    missing = {k: v[0] for k, v in want.items() if k not in got}
    assert not missing, "axis values without a case (smallest geometry of each): %s" % missing
    extra = {k: v for k, v in got.items() if k not in want}
    assert not extra, "cases of values the sweep does not find: %s" % extra
    # the axes the issue names are all there: both outcomes of fusable in the formats that have them, the register bodies
    # with and without a PART 2 launch, PART 0, the table's early-out
    hme = {v for ax, v in want if ax == "hme"}
    for nkbf in (8, 12, 16):
        assert {c[1] for c in hme if c[0] == nkbf} == {"1", "1+2"}, (nkbf, hme)
    assert any(c[0] == 0 and c[1] == "0" for c in hme) and any(c[3] == "early-out" for c in hme)
    assert {v for ax, v in want if ax == "fusable"} >= {(False, FC.F420), (False, FC.F411), (True, FC.F444)}


def test_each_case_is_the_smallest_codable_geometry_of_a_value():
    """every geometry of the list is the first of some value's candidates that is not on a crash list; 1 geometry was excluded that
    way (fwd_cases.ORACLE_DIES), none by tests/golden/ref_crash_skips.json"""
    want = swept()
    excluded = set(FC.ORACLE_DIES)
    assert len(excluded) == 1 and not any(FC.crash_listed(g) for v in want.values() for g in v)
    first = {}
    for k, cands in want.items():
        ok = [g for g in cands if g not in excluded]
        assert ok, "no codable candidate kept for %s: widen fwd_plan.sweep(keep)" % (k,)
        first[k] = ok[0]
    for g in FC.GEOMETRIES:
        assert g in first.values(), "%s is not the smallest geometry of any value" % (g,)
    for k, g in first.items():
        assert g in FC.GEOMETRIES, "%s: smallest codable geometry %s is not a case" % (k, g)
    assert len(set(FC.GEOMETRIES)) == len(FC.GEOMETRIES)


@pytest.mark.parametrize("g", FC.ORACLE_DIES, ids=FC.case_id)
def test_excluded_geometry_still_kills_the_oracle_and_the_reference(g):
    code = ("import sys; sys.path.insert(0, %r); import _cabi as A, fwd_cases as FC; g = %r; "
            "A.orc_encode(FC.make_content(g[0], g[1], g[2], 'dense', FC.seed_of(g)), A.orc_cfg(g[0], g[1], g[2], **FC.cli('dense')), eos=False)"
            % (A.ROOT + "/tests", tuple(g)))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert r.returncode == -8, "the oracle codes %s now (exit %d): make it a candidate again" % (g, r.returncode)
    if A.have_ref():
        # ... as the compiled reference does (its command line on the same clip): there is no answer to be bit-exact with
        import tempfile
        clip = FC.make_content(g[0], g[1], g[2], "dense", FC.seed_of(g))
        kw = FC.cli("dense")
        flags = ["-gop%d" % kw["gop"], "-qp%d" % kw["qp"], "-rc_mode%d" % kw["rc_mode_cli"], "-scd%d" % kw["scd"], "-ipct%d" % kw["ipct"]]
        with tempfile.TemporaryDirectory() as td:
            with pytest.raises(subprocess.CalledProcessError) as e:
                A.ref_cli_encode(clip, g[0], g[1], A.FMT_CLI[g[2]], flags, td)
        assert e.value.returncode == -8, e.value.returncode


def test_block_size_rule_is_the_encoders():
    for h in range(32, 1500, 2):
        for w in (32, 352, 354, 704, 706, 1024, 1026, 1280, 1282, 1400, 4160):
            assert P.block_dims(w, h) == A.block_dims(w, h) and P.block_dims(h, w) == A.block_dims(h, w)


def test_plan_is_the_launchers_decision():
    """dsvg_dispatch_plan runs launch_fwd_sbt's and launch_hme's own decision functions on the geometry tables of an encoder
    context: block size, fusable, strip masks, every motion-search level and the chroma table, on every case and on a sample of the
    sweep in all four formats"""
    pkg = importlib.import_module("digital-subband-video-1_amd")
    rnd = random.Random(0xF0D)
    dom = list(P.sweep_domain())
    sample = [(w, h, fmt) for w, h in rnd.sample(dom, 6000) for fmt in P.FORMATS.values()]
    for g in list(FC.GEOMETRIES) + FC.ORACLE_DIES + sample:
        assert pkg.dispatch_plan(*g) == P.plan(*g).dispatch(), g
    assert pkg.lib().dsvg_dispatch_plan(30, 32, 0, None) != 0


@functools.lru_cache(maxsize=None)
def package():
    pkg = importlib.import_module("digital-subband-video-1_amd")
    L = pkg.lib()
    L.dsvg_fwd_plan.argtypes = [C.c_int] * 6 + [C.c_uint, C.c_int, C.POINTER(pkg.FwdStep), C.c_int, C.POINTER(C.c_int)]
    L.dsvg_hme_plan.argtypes = [C.c_int] * 5 + [C.POINTER(pkg.HmeStep), C.c_int]
    return pkg


@functools.lru_cache(maxsize=None)
def kernel_names():
    L = package().lib()
    return [L.dsvg_prof_kernel_name(i).decode() for i in range(L.dsvg_prof_kernels())]


def plan_geometries():
    """every case, the excluded geometry, and the sample of test_plan_is_the_launchers_decision: 6000 geometries of the sweep's
    domain in all four formats"""
    rnd = random.Random(0xF0D)
    dom = list(P.sweep_domain())
    return list(FC.GEOMETRIES) + FC.ORACLE_DIES + [(w, h, fmt) for w, h in rnd.sample(dom, 6000) for fmt in P.FORMATS.values()]


def fwd_steps(g, group, isP, general_whole=0, switches=0, njobs=1):
    """the product's forward plan (dsvg_fwd_plan): ([FwdStep], mask); the steps are copies, the buffer is the call's own"""
    pkg = package()
    buf, mask = (pkg.FwdStep * 5)(), C.c_int(0)
    n = pkg.lib().dsvg_fwd_plan(g[0], g[1], g[2], group, isP, general_whole, switches, njobs, buf, 5, C.byref(mask))
    assert 1 <= n <= 5, (g, group, isP, n)
    return buf[:n], mask.value


def hme_steps(g, npairs=1, table=1):
    pkg = package()
    buf = (pkg.HmeStep * 14)()
    n = pkg.lib().dsvg_hme_plan(g[0], g[1], g[2], table, npairs, buf, 14)
    assert 1 <= n <= 14, (g, n)
    return buf[:n]


def product_kernels(g, isP, intra):
    """{kernel name: (launches, bytes)} of one picture per frame step, summed over the product's plans in launch order: luma, the
    chroma pair, the step's common launches; a P picture's motion search (a step that continues a bracket opens none)"""
    names, k = kernel_names(), {}
    for group in (0, 1, package().FWD_GROUP_STEP):
        for s in fwd_steps(g, group, isP, intra)[0]:
            P._add(k, names[s.kernel], s.bytes)
    if isP:
        for s in hme_steps(g):
            if not s.cont:
                P._add(k, names[s.kernel], s.bytes)
    return k


def test_plan_steps_are_the_restated_kernels_launches_and_bytes():
    """dsvg_fwd_plan + dsvg_hme_plan, summed per kernel name, are fwd_plan.Plan.i_kernels and p_kernels(intra) for both values of
    intra: launch counts and bytes exactly.  (Every figure is exact: the factors are integers times 3, 3.5, 5, 8 -- dyadic -- or one
    product with 1.4, rounded alike on both sides, and both sides add luma before chroma.)  k_mc is not the forward plan's
    (launch_mc, k_bmc.hip): it is left out of the comparison.  The general kernel's launch count is general_branch's."""
    for g in plan_geometries():
        plan = P.plan(*g)
        assert product_kernels(g, 0, 0) == plan.i_kernels, g
        for intra in (0, 1):
            want = {n: v for n, v in plan.p_kernels(intra).items() if n != P.K_MC}
            assert product_kernels(g, 1, intra) == want, (g, intra)
        for group, pix in ((0, P.K_PIX_Y), (1, P.K_PIX_C)):
            steps, mask = fwd_steps(g, group, 1)
            assert mask == plan.masks[group], g
            n = sum(kernel_names()[s.kernel] == pix for s in steps)
            assert n == (P.general_branch(mask)[1] if plan.fusable else 0), (g, group)


def test_general_kernel_strips_are_the_restated_ladder_and_cover_what_the_lean_kernel_leaves():
    """the general kernel's launches of a P plane group (njobs = 1 and 3): grid, offsets and strides are fwd_plan.general_strips;
    every level-3 patch the lean kernel can leave -- in the first / last patch row / column where the mask names that side, anywhere
    with WHOLE -- lies in a thread block of some launch, every thread block of a launch is one of the full grid, and no step of any
    forward plan has an empty grid"""
    names = kernel_names()
    for g in plan_geometries():
        if not P.fusable(*g):
            continue
        for group, njobs in ((0, 1), (1, 1), (0, 3), (1, 3)):
            _, _, W, H = P.plane_dims(*g)[group]
            w3, h3 = P.rsu(W, 3), P.rsu(H, 3)
            fx, fy, nz = (w3 + 63) // 64, (h3 + 3) // 4, njobs * (2 if group else 1)     # grid3 (k_sbt.hip:3247)
            steps, mask = fwd_steps(g, group, 1, njobs=njobs)
            assert all(min(s.grid) >= 1 and min(s.block) >= 1 for s in steps), (g, group)
            fast, pix = steps[0], steps[1:]
            assert names[fast.kernel] == (P.K_FAST_C if group else P.K_FAST_Y) and tuple(fast.grid) == (fx, fy, nz) and fast.xcd == 1
            assert all(names[s.kernel] == (P.K_PIX_C if group else P.K_PIX_Y) and s.xcd == 0 and s.bytes == 0.0 for s in pix)
            got = [(s.grid[0], s.grid[1]) + tuple(s.args) for s in pix]
            assert got == P.general_strips(mask, fx, fy) and all(s.grid[2] == nz for s in pix), (g, group, mask, got)
            # the thread blocks (columns, rows of the full grid) of every launch
            blocks = set()
            for gx, gy, bxo, byo, bxs, bys in got:
                cells = {(bxo + x * bxs, byo + y * bys) for x in range(gx) for y in range(gy)}
                assert all(0 <= bx < fx and 0 <= by < fy for bx, by in cells), (g, group, got)
                blocks |= cells
            # patch (I, J) is thread (I % 64, J % 4) of thread block (I // 64, J // 4) (k_fwd_mc_pix, k_sbt.hip:1169)
            if mask & P.WHOLE:
                assert blocks == {(bx, by) for bx in range(fx) for by in range(fy)}, (g, group)
            for side, cells in ((P.TOP, {(bx, 0) for bx in range(fx)}), (P.BOTTOM, {(bx, (h3 - 1) // 4) for bx in range(fx)}),
                                (P.LEFT, {(0, by) for by in range(fy)}), (P.RIGHT, {((w3 - 1) // 64, by) for by in range(fy)})):
                if mask & side:
                    assert cells <= blocks, (g, group, mask, side, got)
    for g in list(FC.GEOMETRIES) + FC.ORACLE_DIES:
        for group, isP, sw in [(gr, p, 0) for gr in (0, 1, 2) for p in (0, 1)] + [(0, 1, 2), (1, 1, 2), (2, 0, 4)]:
            assert all(min(s.grid) >= 1 and min(s.block) >= 1 for s in fwd_steps(g, group, isP, switches=sw)[0]), (g, group, isP, sw)


def test_motion_search_steps_are_the_restated_levels():
    """dsvg_hme_plan for 1 and 3 pairs: k_hme_csum where hme_csum says so, then every level from the top down with the launches its
    `parts` names (hme_level) -- PART 3 or 1 in the register body NKBF, PART 2 / 0 in the generic one --, their counts nvx * nvy /
    nfull / nrest, the reciprocals and grids of those counts, one profiler bracket per level; k_hme_detail last"""
    names = kernel_names()

    def uinv(d):
        return min((1 << 32) // max(d, 1), (1 << 32) - 1)                                    # k_hme.hip: hme_plan's uinv

    for g in plan_geometries():
        w, h, fmt = g
        bw, bh, nbh, nbv = P.block_dims(w, h)
        levels = P.pyramid_levels(w, h, nbh, nbv)
        for npairs in (1, 3):
            S = hme_steps(g, npairs)
            csum = P.hme_csum(w, h, fmt)
            if csum:
                s, S = S[0], S[1:]
                assert names[s.kernel] == P.K_HME_CSUM and tuple(s.grid) == (s.fully, 2 * npairs) and s.fully >= 1 and not s.cont, g
            assert names[S[-1].kernel] == P.K_HME_DETAIL and tuple(S[-1].grid) == ((nbh * nbv + 255) // 256, npairs), g
            S = S[:-1]
            assert [s.level for s in S] == sorted((s.level for s in S), reverse=True) and {s.level for s in S} == set(range(levels + 1)), g
            for l in range(levels + 1):
                nkbf, fullx, fully, parts, nrest = P.hme_level(w, h, l)
                step = 1 << l
                nvx, nvy = (nbh + step - 1) // step, (nbv + step - 1) // step
                mine = [s for s in S if s.level == l]
                assert sum(1 << s.part for s in mine) == parts and len({s.part for s in mine}) == len(mine), (g, l)
                assert [s.cont for s in mine] == [0] + [1] * (len(mine) - 1), (g, l)
                for s in mine:
                    count = {0: nvx * nvy, 3: nvx * nvy, 1: fullx * fully, 2: nrest}[s.part]
                    assert (s.l0, s.nkbf, s.count) == (int(l == 0), nkbf if s.part in (1, 3) else 0, count) and count >= 1, (g, l, s.part)
                    assert names[s.kernel] == (P.K_HME_UP if l else P.K_HME_L0) and (s.fullx, s.fully) == (fullx, fully), (g, l)
                    assert (s.inv_per, s.inv_row) == (uinv(count), uinv(fullx if s.part == 1 else nvx)), (g, l, s.part)
                    assert tuple(s.grid) == ((count * npairs + 3) // 4, 1) and s.block == 256, (g, l)      # HME_WPG = 4 waves of NT = 64 (k_hme.hip:42,47)


def test_tail_variant_turns_at_96_workgroups():
    """k_tail_q of a frame step's njobs pictures: 1024 threads up to 96 workgroups (3 * 32), 256 above (3 * 33), as
    fwd_plan.tail_threads says; without the LL quantiser k_fwd_tail, always 256"""
    pkg, names = package(), kernel_names()
    for g in FC.GEOMETRIES[:3]:
        for njobs in (1, 31, 32, 33, 34, 64, 200):
            mid4, tail = fwd_steps(g, pkg.FWD_GROUP_STEP, 0, njobs=njobs)[0]
            assert names[mid4.kernel] == P.K_MID4 and mid4.args[0] == 1 and mid4.grid[2] == 3 * njobs
            assert names[tail.kernel] == P.K_TAIL_Q and tuple(tail.grid) == (3 * njobs, 1, 1), (g, njobs)
            assert tuple(tail.block) == (P.tail_threads(njobs), 1), (g, njobs)
            mid4, tail = fwd_steps(g, pkg.FWD_GROUP_STEP, 0, switches=pkg.FWD_NO_LLQ, njobs=njobs)[0]
            assert mid4.args[0] == 0 and names[tail.kernel] == "k_fwd_tail" and tuple(tail.block) == (256, 1), (g, njobs)
    assert P.tail_threads(32) == 1024 and P.tail_threads(33) == 256
    assert pkg.lib().dsvg_fwd_plan(30, 32, 0, 0, 1, 0, 0, 1, None, 0, None) < 0 and pkg.lib().dsvg_hme_plan(30, 32, 0, 1, 1, None, 0) < 0


@pytest.mark.parametrize("g", FC.GEOMETRIES, ids=FC.case_id)
def test_contents_do_what_they_are_there_for(g, orc):
    """on the oracle's motion fields: ONE P picture of the motion content has all four half-pel phases, a non-zero vector at
    blocks of every edge and, at every edge, an inter block whose vector points out of the picture -- at every geometry of the
    list, the pictures of 2x2 blocks included; the intra content (where the geometry runs it) has intra blocks in every P
    picture; dense and sparse are inv_cases' contents"""
    w, h, fmt = g
    assert "motion" in FC.contents_of(g) and "dense" in FC.contents_of(g)
    clip = FC.make_content(w, h, fmt, "motion", FC.seed_of(g))
    facts = [FC.field_facts(f, w, h) for f in FC.oracle_fields(clip, w, h, fmt, **FC.cli("motion"))]
    assert len(facts) == FC.NFRAMES - 1
    assert any(len(ph) == 4 and out == set("LRTB") and nz == set("LRTB") for ph, out, nz, _ in facts), (g, facts)
    if "intra" in FC.contents_of(g):
        clip = FC.make_content(w, h, fmt, "intra", FC.seed_of(g))
        facts = [FC.field_facts(f, w, h) for f in FC.oracle_fields(clip, w, h, fmt, **FC.cli("intra"))]
        assert all(f[3] > 0 for f in facts), (g, [f[3] for f in facts])


def test_every_strip_case_runs_all_four_contents():
    """contents are cut only where the motion search's classes live (64-wide blocks); every value of the luma, chroma and fusable
    axes has a case with all four"""
    for (ax, v), gs in case_values().items():
        if ax != "hme":
            assert any(FC.contents_of(g) == list(FC.CONTENTS) for g in gs), (ax, v, gs)
