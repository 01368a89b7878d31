"""CPU: the model of the entropy decoder (tests/hzdec_plan.py) against the oracle and, where it is built, the compiled reference,
and the coverage of its labels by the cases of tests/hzdec_cases.py.  Nothing of the product is loaded.

  * on every case the model's reader (the reference's rules in Python integers) gives the plane orc_decode_plane gives, and
    dsv_decode_plane where oracle/_ref holds the reference;
  * on every case the model's restatement of the KERNELS' decomposition (chunks, entering states, code ends, cbase, prev_end,
    k_hz_codes' arithmetic, the 64-bit position sum) arrives at the reader's entry list: the algorithm is checked here, the
    device only has to execute it;
  * every label outside UNREACHABLE is reached by a case that names it, every case reaches the labels it names;
  * the constants the model restates are the kernels';
  * a flipped rule of the reader (truncation comparison, later region wins, the + 1 between runs) is noticed.
"""
import os
import re

import numpy as np
import pytest

import _cabi as A
import hz_plan as H
import hzdec_cases as DC
import hzdec_plan as D

OP = DC.op_cases()
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "digital-subband-video-1_amd", "csrc")
SEAM_OP = {"sc.i32"}                        # the operator decodes into int32 coefficients (dec_sym == 0) and never clears


@pytest.fixture(scope="module")
def want(orc):
    """the oracle's plane per case, computed once"""
    return {name: DC.decode(orc, "orc_decode_plane", c) for name, c in OP.items()}


@pytest.mark.parametrize("name", list(OP))
def test_case(orc, want, name):
    c = OP[name]
    m = DC.model_of(name)
    dc, entries = D.read_entries(c["buf"], c["len"], m.nscan)
    got = D.coef_plane(c["w"], c["h"], dc, entries, DC.OP_Q)
    assert np.array_equal(got, want[name]), "%s: the model's reader and the oracle disagree: %s" % (name, m.explain(got, want[name]))
    if A.have_ref():
        A.assert_same("%s: oracle against the compiled reference" % name, want[name], DC.decode(A.load_ref(), "dsv_decode_plane", c), (c["h"], c["w"]))
    assert (m.dc, m.entries) == (dc, entries), "%s: the kernels' decomposition decodes %d entries, the reader %d; first difference %s" % (
        name, len(m.entries), len(entries), next((i for i, (a, b) in enumerate(zip(m.entries, entries), 1) if a != b), min(len(m.entries), len(entries)) + 1))
    assert m.labels <= set(D.LABELS), m.labels - set(D.LABELS)
    assert set(c["labels"]) <= m.labels | SEAM_OP, "%s is listed for %s" % (name, sorted(set(c["labels"]) - m.labels))
    # the payload is one the reference defines: the buffer ends in guard bytes it never needed
    assert c["buf"][-DC.GUARD:] == b"\xff" * DC.GUARD and c["len"] <= c["plen"]
    assert all(ch.keep > 0 for ch in m.chunks) and len(m.chunks) <= c["len"] // 16 + 2, "the hand-over records fit what the launchers allocate"


def test_every_label_is_reached():
    """a condition, not a measurement: no label may be left out"""
    named = {}
    for name, c in OP.items():
        for l in set(c["labels"]) & (DC.model_of(name).labels | SEAM_OP):
            named.setdefault(l, name)
    for call in DC.PIPE_CALLS.values():
        for l in call["labels"]:
            named.setdefault(l, "pipeline")
    assert set(D.UNREACHABLE) <= set(D.LABELS)
    missing = set(D.LABELS) - set(D.UNREACHABLE) - set(named)
    assert not missing, "no case names and reaches %s" % sorted(missing)
    reached = set().union(*(DC.model_of(n).labels for n in OP))
    assert not (reached & set(D.UNREACHABLE)), "declared unreachable, but reached: %s" % sorted(reached & set(D.UNREACHABLE))


def test_pipeline_calls_reach_their_labels():
    """the call-level labels come from call_labels, the plane-level ones from the model of the spliced planes"""
    for name, call in DC.PIPE_CALLS.items():
        got = D.call_labels(call["kinds"], call["sym"], call.get("lens"), call.get("sym_i", True))
        for pl in call.get("planes", ()):
            got |= D.Plane(pl["w"], pl["h"], pl["buf"], pl["plen"]).labels
        assert set(call["labels"]) <= got, "%s is listed for %s" % (name, sorted(set(call["labels"]) - got))


@pytest.mark.parametrize("plane", [0, 1, 2])
def test_the_dc_cell_case_sees_the_dc(orc, plane):
    """the pipeline case that decides who wins the DC's cell must depend on it: a decoder in which entry 1's symbol wins decodes
    the plane 'pos0-dc-lost', and the oracle's frame for that plane differs from the expected one in most of the plane's samples"""
    w, h, fmt = DC.PIPE_G
    want = A.orc_decode(b"".join(DC.spliced(DC.PIPE_G, "IP", DC.POS0_SEED, [(1, plane, "pos0")])), w, h, fmt)
    lost = A.orc_decode(b"".join(DC.spliced(DC.PIPE_G, "IP", DC.POS0_SEED, [(1, plane, "pos0-dc-lost")])), w, h, fmt)
    assert len(want) == len(lost) == 2 and np.array_equal(want[0], lost[0])
    differ = int((np.asarray(want[1]) != np.asarray(lost[1])).sum())
    assert differ > w * h // 2, "only %d samples of the frame depend on the DC of plane %d" % (differ, plane)


def _define(name):
    for f in ("k_hzcc.hip", "dsvg_dev.hpp"):
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, open(os.path.join(CSRC, f)).read(), re.M)
        if m:
            return int(m.group(1))
    raise AssertionError("%s is not defined by name in csrc/k_hzcc.hip or the header it includes" % name)


def test_constants_are_the_kernels():
    for name in ("PARSE_THREADS", "PARSE_BITS", "HZ_CHUNK", "POS_ITEMS"):
        assert _define(name) == getattr(D, name), name
    assert D.HZ_CHUNK == H.HZ_CHUNK and D.PASS_BITS == 131072
    src = open(os.path.join(CSRC, "k_hzcc.hip")).read()
    assert "base += PARSE_THREADS * POS_ITEMS" in src and "tid * POS_ITEMS" in src, "k_hz_positions walks POS_ITEMS entries per thread"


def test_machine_is_parse_step():
    """the five states on the codes of bs.c:129-206: U(2) N(-3) = 011 0111 ends after bits 2 and 6"""
    st, ends = 0, []
    for i, b in enumerate([0, 1, 1, 0, 1, 1, 1]):
        st, e = D.STEP[st][b]
        if e:
            ends.append(i)
    assert ends == [2, 6] and st == 0


def test_geometry_of_the_cases():
    assert H.geometry(*DC.CIF)[1] == 101376 and H.geometry(8, 8)[1:] == (64, 1) and H.geometry(16, 16)[2] == 1
    assert H.geometry(*DC.WIDE)[1] == 147456 and not H.overlaps(*DC.WIDE)
    assert H.overlaps(*DC.OVERLAP) and not H.overlaps(64, 64) and not H.overlaps(*DC.CIF)


@pytest.mark.parametrize("rule,cases", [("trunc_ge", ["cut-val-7b", "cut-last-7b"]), ("later_wins", ["shared-both-01", "shared-both-12"]), ("plus1", ["pos0", "states"])])
def test_a_flipped_rule_is_noticed(want, rule, cases):
    """each of the reader's three rules decides some case's plane"""
    for name in cases:
        c = OP[name]
        rules = dict(D.RULES, **{rule: False})
        dc, entries = D.read_entries(c["buf"], c["len"], DC.model_of(name).nscan, rules)
        assert not np.array_equal(D.coef_plane(c["w"], c["h"], dc, entries, DC.OP_Q, rules=rules), want[name]), "%s does not depend on %s" % (name, rule)
