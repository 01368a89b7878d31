"""The case table of tests/hme_cases.py, proven on the CPU: nothing of the product runs here.

  * every case reaches every label it lists, and every label of hme_plan.LABELS is reached by some case -- or is in hme_plan.UNREACHABLE,
    whose entries each carry the line that makes them impossible and a condition on the kernel's constants that is checked here;
  * on every case the oracle's fields, every level and every field, are the reference's (run beside it where oracle/_ref was built, and
    against its stored answers in tests/golden/ref_answers.json everywhere): the built inputs are unusual enough to pin the restatement
    on them;
  * on every case the pixels the reference's code touches -- scored candidates, the nine points, the lattice's 19x20 patch, the windows:
    all derived from the trace -- lie inside the bordered frames.  Beyond the border the reference reads what its heap holds, and a
    parity test there proves nothing: such a case is rebuilt, not exempted.

The dispatch branch that needs a picture wider than 4096 pixels (k_hme_csum returning at once for more than 64 full block columns, csum
"early-out") stays with the 4160-wide cases of fwd_cases.py; hme_plan.ELSEWHERE names it."""
import ctypes as C

import numpy as np
import pytest

import _cabi as A
import fwd_plan
import hme_cases as H
import hme_plan as P

IDS = [c.name for c in H.CASES]
FIELDS = ("x", "y", "mode", "submask", "lo_var", "lo_tex", "high_detail")


@pytest.fixture(scope="module")
def ref():
    return A.load_ref() if A.have_ref() else None


@pytest.fixture(scope="module")
def traced(orc):
    """per case: (source frames, reference frames, intra %, fields, trace, labels per block over the case's operator calls)"""
    out = []
    for c in H.CASES:
        src, rf = c.build()
        pct, fields, tr = P.run_oracle(orc, c.geo, src, rf)
        out.append((src, rf, pct, fields, tr, P.labels_of(c.geo, tr, src, rf, c.flags())))
    return out


def test_the_table_is_well_formed():
    assert len(set(IDS)) == len(IDS)
    for c in H.CASES:
        g = c.geo
        assert g.w <= 384 and g.h <= 256, c.name
        assert c.labels, c.name
        for k in c.labels:
            assert k in P.LABELS, (c.name, k)
        # the reference divides by the chroma block's area (c_maxvar hme.c:269-300): no partial block may lose its chroma
        for _, _, _, _, bw, bh in H.blocks(g, 0):
            assert bw >> g.hs and bh >> g.vs, (c.name, bw, bh)
    for k, (why, holds) in P.UNREACHABLE.items():
        assert k in P.LABELS and why[0].isdigit(), k
        assert holds(), "the condition that makes %s unreachable no longer holds: %s" % (k, why)
    for k, where in P.LABELS.items():
        assert where[0].isdigit() or where.startswith("hme.c:"), (k, where)


@pytest.mark.parametrize("n", range(len(H.CASES)), ids=IDS)
def test_case_reaches_its_labels(traced, n):
    c = H.CASES[n]
    reached = set().union(*traced[n][5].values())
    assert not set(reached) - set(P.LABELS), sorted(set(reached) - set(P.LABELS))
    missing = [k for k in c.labels if k not in reached]
    assert not missing, "%s no longer reaches %s" % (c.name, missing)


def test_every_label_is_reached_or_proven_unreachable(traced):
    reached = set()
    for t in traced:
        reached |= set().union(*t[5].values())
    listed = set(k for c in H.CASES for k in c.labels)
    assert not [k for k in P.LABELS if k not in reached and k not in P.UNREACHABLE], [k for k in P.LABELS if k not in reached and k not in P.UNREACHABLE]
    assert not [k for k in P.UNREACHABLE if k in reached], "reached after all: take them out of UNREACHABLE"
    assert not [k for k in P.LABELS if k not in listed and k not in P.UNREACHABLE], "reached, but no case is there for: %s" % sorted(set(P.LABELS) - listed - set(P.UNREACHABLE))
    # the one dispatch branch left to the wide cases of fwd_cases.py is really there
    assert P.ELSEWHERE == ("csum.early-out",)
    import fwd_cases
    assert any(w > 4096 and fwd_plan.hme_csum(w, h, fmt) == 2 for w, h, fmt in fwd_cases.GEOMETRIES)


@pytest.mark.parametrize("n", range(len(H.CASES)), ids=IDS)
def test_oracle_is_the_reference_on_the_case(ref, traced, n):
    c, g = H.CASES[n], H.CASES[n].geo
    src, rf, pct, fields, tr, _ = traced[n]
    want = None
    if ref:
        meta = A.Meta(g.w, g.h, g.fmt, 30, 1, 1, 1)
        prm = A.Params(C.pointer(meta), 1, 1, g.bw, g.bh, g.nxb, g.nyb)
        hm = A.HME()
        hm.params = C.pointer(prm)
        hm.levels = g.levels
        for l in range(g.levels + 1):
            hm.src[l] = C.pointer(src[l].c)
            hm.ref[l] = C.pointer(rf[l].c)
        rp = ref.dsv_hme(C.byref(hm))
        want = []
        for l in range(g.levels + 1):
            want.append(np.ctypeslib.as_array(C.cast(hm.mvf[l], C.POINTER(C.c_uint8)), shape=(g.nblk * 12,)).copy().view(A.MV_DTYPE))
            ref.dsv_free(C.cast(hm.mvf[l], C.c_void_p))
    key = "hme_case/" + c.name
    A.check_ref(key + "/intra_pct", rp if ref else None, pct)
    for l in range(g.levels + 1):
        if ref:
            for k in FIELDS:
                bad = np.nonzero(want[l][k] != fields[l][k])[0]
                assert not bad.size, "oracle differs from the reference: " + P.explain(g, traced[n][5], l, int(bad[0]), k, fields[l][k][bad[0]], want[l][k][bad[0]])
        A.known_answer("%s/mv_level%d" % (key, l),
                       np.concatenate([np.ascontiguousarray((want[l] if ref else fields[l])[k]).view(np.uint8).ravel() for k in FIELDS]))
    # the trace is the search's own: the vectors it recorded are the fields'
    for l in range(g.levels + 1):
        v = tr[l]["visited"] == 1
        assert np.array_equal(tr[l]["mvx"][v], fields[l]["x"][v]) and np.array_equal(tr[l]["mvy"][v], fields[l]["y"][v])


@pytest.mark.parametrize("n", range(len(H.CASES)), ids=IDS)
def test_reads_stay_inside_the_bordered_frames(traced, n):
    g = H.CASES[n].geo
    tr = traced[n][4]
    for l in range(g.levels + 1):
        fw, fh = g.dims[l]
        for b in np.nonzero(tr[l]["visited"] == 1)[0]:
            for frame, (x0, y0, x1, y1) in P.reads(g, tr[l, b]):
                assert -P.BORDER <= x0 and -P.BORDER <= y0 and x1 <= fw + P.BORDER and y1 <= fh + P.BORDER, \
                    "%s level %d block %d reads %s pixels (%d, %d) .. (%d, %d) of a %dx%d picture" % (g.name, l, b, frame, x0, y0, x1, y1, fw, fh)


def test_trace_leaves_the_search_alone(orc):
    """orc_hme_run with and without the trace: the same fields, the same counters"""
    c = H.CASES[IDS.index("mix-16")]
    src, rf = c.build()
    orc.orc_cov_read.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    out = []
    for traced_run in (False, True):
        orc.orc_cov_reset()
        if traced_run:
            pct, fields, _ = P.run_oracle(orc, c.geo, src, rf)
        else:
            g = c.geo
            meta = A.Meta(g.w, g.h, g.fmt, 30, 1, 1, 1)
            prm = A.Params(C.pointer(meta), 1, 1, g.bw, g.bh, g.nxb, g.nyb)
            hm = A.HME()
            hm.params = C.pointer(prm)
            hm.levels = g.levels
            for l in range(g.levels + 1):
                hm.src[l] = C.pointer(src[l].c)
                hm.ref[l] = C.pointer(rf[l].c)
            pct = orc.orc_hme_run(C.byref(hm))
            fields = []
            for l in range(g.levels + 1):
                fields.append(np.ctypeslib.as_array(C.cast(hm.mvf[l], C.POINTER(C.c_uint8)), shape=(g.nblk * 12,)).copy())
                C.CDLL(None).free(hm.mvf[l])
        v = (C.c_ulonglong * 64)()
        orc.orc_cov_read(v, 64)
        out.append((pct, [np.asarray(f).view(np.uint8).tobytes() for f in fields], list(v)))
    assert out[0] == out[1]
