"""CPU checks of the forward / motion-search matrix (tests/fwd_cases.py) against the restated dispatch (tests/fwd_plan.py).

The matrix must hold one case of every value of every axis the sweep finds, each the smallest geometry of its value that the
oracle codes, so a new branch of launch_fwd_sbt or launch_hme fails here until a case is added.  The restatement is compared with
the launchers' own decision functions (dsvg_dispatch_plan: no device needed) on every case and on a sample of the sweep; that the
kernels then ran as planned is checked on the GPU (tests/test_gpu_fwd_paths.py).  The contents must do on the oracle's streams
what they are there for."""
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
