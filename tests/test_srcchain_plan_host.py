"""The decisions of a session's source side (csrc/host/dsv1_srcchain_plan.h through dsv1_srcchain_plan_set / _call, no device) against
their restatement (tests/srcchain_plan.py), exhaustively: from the empty chain every reachable state is walked breadth-first, at every
state every request is tried (set, change and clear of every pass, valid and not, the three resets, the seek; busy and not) and every
call form planned, over F in {4, 6}, 4:2:0 and 4:2:2, a session that keeps its lane and one that does not.  The invariants of a call's
steps and of the clips' sizes over every state; and every row of the refusal table must have been produced."""
import collections
import ctypes as C
import importlib

import pytest

import _cabi as A
import srcchain_plan as R

W, H, NSRC = 64, 48, 2
IN_W, IN_H = 80, 60                     # the reframe's input
KINDS = {"conv": 1, "levels": 2, "deint": 3, "ivtc": 4, "denoise": 5, "orient": 6, "reframe": 7, "overlays": 8}
OPS = {"set": 0, "reset": 1, "seek": 2}
# the restatement's reasons -> words the row of the library's table must hold
REASON_WORDS = {
    "source": "no such source", "field_F": "even frames_per_call", "ivtc_F": "multiple of 4",
    "busy": "in flight", "not_set": "not set", "deint_while_ivtc": "a deinterlacer while an inverse telecine",
    "ivtc_while_deint": "an inverse telecine while a deinterlacer", "reframe_while_front": "a reframe while a source format",
    "reframe_while_orient": "a reframe while an orientation", "orient_while_front": "an orientation while a source format",
    "invalid_conv": "not a valid pixel or RGB format", "invalid_deint": "not a deinterlacer",
    "invalid_ivtc": "not an inverse telecine", "invalid_denoise": "not a noise filter", "invalid_orient": "not an orientation",
    "invalid_reframe": "not a valid reframe", "invalid_overlays": "not a valid list of overlays"}


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("digital-subband-video-1_amd")
    p.lib()
    return p


def c_state(pkg, c):
    s = pkg.SrcChainState(nsrc=c["nsrc"], F=c["F"], subsamp=c["subsamp"], keep_lane=c["keep_lane"], ow=c["ow"], oh=c["oh"])
    t = c["temporal"]
    kinds = [1 if c["conv"] else 0, 2 if c["levels"] else 0, 0 if not t else 3 if t[0] == "deint" else 4, 5 if c["denoise"] else 0,
             6 if c["orient"] else 0, 7 if c["reframe"] else 0, 8 if c["overlays"] else 0]
    for p, k in enumerate(kinds):
        s.kind[p] = k
    if c["conv"]:
        s.conv_rgb, s.conv_fb = int(c["conv"][0] == "rgb"), c["conv"][1]
    if t and t[0] == "deint":
        s.deint_mode = t[1]
    s.orient = c["orient"]
    if c["reframe"]:
        s.in_w, s.in_h = c["reframe"]
    s.ov_clip[0], s.ov_clip[1] = int(c["ov_clip"][0]), int(c["ov_clip"][1])
    return s


def py_state(s):
    """a SrcChainState as the restatement's dict"""
    k = list(s.kind)
    return dict(nsrc=s.nsrc, F=s.F, subsamp=s.subsamp, keep_lane=s.keep_lane, ow=s.ow, oh=s.oh,
                conv=("rgb" if s.conv_rgb else "pix", s.conv_fb) if k[0] else None, levels=k[1] == 2,
                temporal=("deint", s.deint_mode) if k[2] == 3 else ("ivtc",) if k[2] == 4 else None, denoise=k[3] == 5,
                orient=s.orient if k[4] else 0, reframe=(s.in_w, s.in_h) if k[5] else None, overlays=k[6] == 8,
                ov_clip=[bool(s.ov_clip[0]), bool(s.ov_clip[1])])


def c_req(pkg, q):
    r = pkg.SrcChainReq(op=OPS[q["op"]], kind=KINDS.get(q["kind"], 0), busy=q["busy"], source=q.get("source", 0), valid=1)
    if q["op"] != "set":
        return r
    v, k = q["value"], q["kind"]
    r.set, r.valid, r.identity = int(v is not None or k == "orient"), int(q.get("valid", True)), int(q.get("identity", False))
    if k == "conv" and v:
        r.mode, r.frame_bytes = int(v[0] == "rgb"), v[1]
    if k in ("deint", "orient") and v is not None:
        r.mode = v
    if k == "reframe" and v:
        r.w, r.h, r.out_w, r.out_h = v
    return r


def requests(c):
    """every request tried at state c (busy left to the caller)"""
    g = R.geometry(c)
    out = []
    for v, extra in [(("pix", 2 * g["fb"]), {}), (("rgb", 3 * g["w"] * g["h"]), {}), (("pix", 2 * g["fb"]), {"valid": False}), (None, {})]:
        out.append(dict(op="set", kind="conv", value=v, **extra))
    for v, extra in [(True, {}), (True, {"identity": True}), (True, {"valid": False}), (None, {})]:
        out.append(dict(op="set", kind="levels", value=v, **extra))
    for v, extra in [(0, {}), (1, {}), (0, {"valid": False}), (None, {})]:
        out.append(dict(op="set", kind="deint", value=v, **extra))
    for kind in ("ivtc", "denoise", "overlays"):
        for v, extra in [(True, {}), (True, {"valid": False}), (None, {})]:
            out.append(dict(op="set", kind=kind, value=v, **extra))
    for v in (0, 1, 5, 9):              # none, a mirror, a rotation by 90 degrees, no code
        out.append(dict(op="set", kind="orient", value=v))
    for v, extra in [((IN_W, IN_H, W, H), {}), ((IN_W, IN_H, W // 2, H // 2), {}), ((W, H, W, H), {"identity": True}),
                     ((IN_W, IN_H, W, H), {"valid": False}), (None, {})]:
        out.append(dict(op="set", kind="reframe", value=v, **extra))
    for kind in ("deint", "ivtc", "denoise"):
        for source in (-1, 0, NSRC):
            out.append(dict(op="reset", kind=kind, source=source))
    for kind, source in (("overlays", 1), ("overlays", -2)):
        out.append(dict(op="seek", kind=kind, source=source))
    return out


def key(c):
    return (c["conv"], c["levels"], c["temporal"], c["denoise"], c["orient"], c["reframe"], c["overlays"])


GEOM_FIELDS = ("w", "h", "mw", "mh", "ow", "oh", "conv_frames", "frames_in", "fb", "mfb", "ofb", "frame_in_bytes", "bytes_in")


def check_set(pkg, c, cs, q, texts, seen):
    want = R.plan_set(c, q)
    try:
        got = pkg.srcchain_plan_set(cs, c_req(pkg, q))
    except pkg.SrcChainRefused as e:
        assert want["rc"] == e.rc == R.ERR_ARG and want["reason"], (c, q, e.text)
        assert REASON_WORDS[want["reason"]] in e.text and e.text == texts[e.row], (c, q, want["reason"], e.text)
        seen[e.row] += 1
        return None
    assert want["rc"] == 0 and not want["reason"], (c, q, want["reason"])
    assert bool(got.noop) == want["noop"], (c, q)
    assert py_state(got.next) == want["next"], (c, q, py_state(got.next), want["next"])
    assert {f: getattr(got.g, f) for f in GEOM_FIELDS} == {f: want["geom"][f] for f in GEOM_FIELDS}, (c, q)
    assert bool(got.g.lane) == want["geom"]["lane"], (c, q)
    assert list(got.alloc) == want["alloc"] and [bool(v) for v in got.free_] == want["free"], (c, q, list(got.alloc), want["alloc"])
    assert [bool(v) for v in got.reset] == want["reset"], (c, q, list(got.reset), want["reset"])
    # clip bytes = frame bytes of the position's geometry x sources x frames
    g = want["geom"]
    for p, n in enumerate(got.alloc):
        if n:
            fb = (g["fb"], g["fb"], g["fb"], g["fb"], g["mfb"], g["ofb"])[p]
            assert n == fb * NSRC * (g["conv_frames"] if p < 2 else c["F"]), (c, q, p)
    return want


STEP_KIND = {0: "copy", 1: "conv", 2: "levels", 3: "deint", 4: "ivtc", 5: "denoise", 6: "orient", 7: "reframe", 8: "overlays"}


def check_call(pkg, c, form, active, par):
    want = R.plan_call(c, form, active, par)
    try:
        got = pkg.srcchain_plan_call(c_state(pkg, c), form, active, par)
    except pkg.SrcChainRefused as e:
        assert want["rc"] == e.rc == R.ERR_ARG, (c, form, active)
        return
    assert want["rc"] == 0, (c, form, active)
    steps = [(STEP_KIND[s.kind], s.nframes, s.src, s.dst, s.bytes, s.alloc) for s in got.step[:got.nsteps]]
    assert (bool(got.bypass), got.upload, steps, got.out, got.advance) == (want["bypass"], want["upload"], want["steps"], want["out"], want["advance"]), (c, form, active, steps, want)
    # invariants
    cur = R.UPLOAD if got.upload else R.CALLER
    for kind, n, src, dst, nbytes, alloc in steps:
        assert src == cur, (c, form, active, steps)              # the previous step's destination, or the input
        assert dst != R.CALLER and (form == 0 or dst != R.UPLOAD), (c, form, active, steps)    # a caller's clip is never written
        assert n > 0
        cur = dst
    assert got.out == cur
    assert bool(got.bypass) == (not steps and not got.upload), (c, form, active)       # bypass iff nothing is enqueued
    if got.bypass:
        assert got.out == R.CALLER
    assert got.advance == (c["F"] if c["overlays"] else 0)
    assert got.upload == (0 if form or got.bypass else R.geometry(c)["bytes_in"])


def walk(pkg, F, subsamp, keep_lane, texts, seen):
    """breadth-first from the empty chain: (states, transitions) visited"""
    start = R.empty(NSRC, F, subsamp, keep_lane, W, H)
    states, queue, ntrans = {key(start): start}, collections.deque([start]), 0
    while queue:
        c = queue.popleft()
        cs = c_state(pkg, c)
        for q in requests(c):
            for busy in (0, 1):
                q["busy"] = busy
                want = check_set(pkg, c, cs, q, texts, seen)
                ntrans += 1
                if want and key(want["next"]) not in states:
                    states[key(want["next"])] = want["next"]
                    queue.append(want["next"])
        # (the overlay pass's own clips come and go with calls, not with requests: both cases at every state that has overlays)
        for ov_clip in ([False, False], [True, False]) if c["overlays"] else ([False, False],):
            cc = dict(c, ov_clip=ov_clip)
            for form in (0, 1, 2):
                for active in (False, True):
                    check_call(pkg, cc, form, active, 0)
            if c["overlays"]:
                want = check_set(pkg, cc, c_state(pkg, cc), dict(op="set", kind="overlays", value=None, busy=0), texts, seen)
                assert want["free"][6] == any(ov_clip) and want["next"]["ov_clip"] == [False, False]
    return len(states), ntrans


def test_every_reachable_state_every_request_every_call(pkg):
    texts = pkg.srcchain_plan_texts()
    seen = collections.Counter()
    for F in (4, 6):
        for subsamp in (A.SUBSAMP_420, A.SUBSAMP_422):
            for keep_lane in (0, 1):
                before = collections.Counter(seen)
                nstates, ntrans = walk(pkg, F, subsamp, keep_lane, texts, seen)
                print("F=%d subsamp=0x%x keep_lane=%d: %d states, %d transitions" % (F, subsamp, keep_lane, nstates, ntrans))
                # every combination of the axes is reachable: converter x levels x deinterlacer / IVTC x denoise x orientation x reframe x overlays
                full = 3 * 2 * (4 if F % 4 == 0 else 3) * 2 * (3 if subsamp == A.SUBSAMP_420 else 2) * 2 * 2
                assert nstates == full, (nstates, full)
                new = seen - before
                assert F % 4 == 0 or new[texts.index("inverse telecine needs a frames_per_call that is a multiple of 4")]
                assert subsamp == A.SUBSAMP_420 or new[[i for i, t in enumerate(texts) if "not an orientation" in t][0]]
    # (both F of the walks are even: the two rules on F once more at an odd one)
    odd = R.empty(NSRC, 5, A.SUBSAMP_420, 0, W, H)
    for q in (dict(op="set", kind="deint", value=1, busy=0), dict(op="set", kind="deint", value=0, busy=0), dict(op="set", kind="ivtc", value=True, busy=0)):
        check_set(pkg, odd, c_state(pkg, odd), q, texts, seen)
    dead = [t for i, t in enumerate(texts) if t and not seen[i]]
    assert not dead, "refusal rows never produced: %s" % dead
    print("%d refusal rows, each produced" % len([t for t in texts if t]))


def test_a_refusal_changes_nothing(pkg):
    """the plan of a refused request is the state it was asked about, with nothing to allocate, free or forget"""
    c = R.empty(NSRC, 4, A.SUBSAMP_420, 0, W, H)
    c["denoise"] = True
    cs = c_state(pkg, c)
    out = pkg.SrcChainSetPlan()
    q = c_req(pkg, dict(op="set", kind="reframe", value=(IN_W, IN_H, W, H), busy=0))
    assert pkg.lib().dsv1_srcchain_plan_set(C.byref(cs), C.byref(q), C.byref(out)) == R.ERR_ARG
    assert py_state(out.next) == c and not any(out.alloc) and not any(out.free_) and not any(out.reset) and not out.noop
    assert out.g.w == W and out.g.lane == 1
    for q in (dict(op="reset", kind="conv", source=0, busy=0), dict(op="seek", kind="levels", source=0, busy=0), dict(op="set", kind="none", value=None, busy=0)):
        with pytest.raises(ValueError, match="not a request"):
            pkg.srcchain_plan_set(cs, c_req(pkg, q))
