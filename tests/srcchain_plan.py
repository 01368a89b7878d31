"""The source side of a session restated from its documented rules ("The source side of a session"; include/dsv1_api.h,
the setters' comments and "Source chain plan"), not from csrc/host/dsv1_srcchain_plan.h: what a setter, a reset or a seek call is
answered with, and what one call enqueues.  tests/test_srcchain_plan_host.py holds the library's two queries to it.

A chain here is a dict: nsrc, F, subsamp, keep_lane, ow, oh (the canvas), and what is set --
  conv: None | ("pix", frame_bytes) | ("rgb", frame_bytes);  levels: bool;  temporal: None | ("deint", mode) | ("ivtc",);
  denoise: bool;  orient: code (0: none);  reframe: None | (in_w, in_h);  overlays: bool;  ov_clip: [bool, bool].
A request is a dict: op "set" | "reset" | "seek", kind (a name of ORDER or "deint" / "ivtc"), busy, and for a set: value (None
clears) with valid / identity where the pass has such a notion; source for reset and seek."""
ORDER = ["conv", "levels", "temporal", "denoise", "orient", "reframe", "overlays"]       # the chain, front to back
POS = {"conv": 0, "levels": 1, "deint": 2, "ivtc": 2, "denoise": 3, "orient": 4, "reframe": 5, "overlays": 6}
DEINT_FIELD = 1
ERR_ARG = -2


def frame_bytes(w, h, subsamp):
    hs, vs = (subsamp >> 2) & 3, subsamp & 3
    return w * h + 2 * (-(-w // (1 << hs))) * (-(-h // (1 << vs)))


def empty(nsrc, F, subsamp, keep_lane, ow, oh):
    return dict(nsrc=nsrc, F=F, subsamp=subsamp, keep_lane=keep_lane, ow=ow, oh=oh, conv=None, levels=False, temporal=None,
                denoise=False, orient=0, reframe=None, overlays=False, ov_clip=[False, False])


def is_set(c, slot):
    return bool(c[slot])


def geometry(c):
    """the three geometries, what a call brings, whether a lane exists"""
    mw, mh = c["reframe"] if c["reframe"] else (c["ow"], c["oh"])
    w, h = (mh, mw) if c["orient"] & 4 else (mw, mh)        # the inverse of a transposing code transposes
    ivtc = c["temporal"] == ("ivtc",)
    field = c["temporal"] == ("deint", DEINT_FIELD)
    g = dict(w=w, h=h, mw=mw, mh=mh, ow=c["ow"], oh=c["oh"])
    g["fb"], g["mfb"], g["ofb"] = frame_bytes(w, h, c["subsamp"]), frame_bytes(mw, mh, c["subsamp"]), frame_bytes(c["ow"], c["oh"], c["subsamp"])
    g["conv_frames"] = c["F"] // 4 * 5 if ivtc else c["F"]
    g["frames_in"] = c["F"] // 4 * 5 if ivtc else c["F"] // 2 if field else c["F"]
    g["frame_in_bytes"] = c["conv"][1] if c["conv"] else g["fb"]
    g["bytes_in"] = g["frame_in_bytes"] * c["nsrc"] * g["frames_in"]
    g["lane"] = bool(c["keep_lane"] or any(is_set(c, s) for s in ORDER))
    return g


def clip_bytes(c, g, pos):
    """each of the two clips of the pass at a position: frame bytes of that position's geometry x sources x frames"""
    fb = g["fb"] if pos <= 3 else g["mfb"] if pos == 4 else g["ofb"]
    return fb * c["nsrc"] * (g["conv_frames"] if pos <= 1 else c["F"])


def refusal(c, q):
    """the reason of the first refusal in the stated order -- validity, busy, exclusion -- or None"""
    kind, front = q["kind"], any(is_set(c, s) for s in ORDER[:4])
    # (a reset is for the passes with a history or a state, a seek for the overlays: anything else is no request)
    assert q["op"] == "set" and kind in POS or q["op"] == "reset" and kind in ("deint", "ivtc", "denoise") or q["op"] == "seek" and kind == "overlays"
    if q["op"] in ("reset", "seek"):
        if not -1 <= q["source"] < c["nsrc"]:
            return "source"
        if q["op"] == "reset" and q["busy"]:
            return "busy"
        if q["op"] == "seek":
            return None if c["overlays"] else "not_set"
        return None if c["temporal"] and c["temporal"][0] == kind or (kind == "denoise" and c["denoise"]) else "not_set"
    v = q["value"]
    if kind == "orient":
        if not 0 <= v < 8 or (v & 4 and ((c["subsamp"] >> 2) & 3) != (c["subsamp"] & 3)):
            return "invalid_orient"
    elif v is not None:
        if not q.get("valid", True) and kind != "levels":    # (every levels table is a setting)
            return "invalid_" + kind
        if kind == "conv" and not v[1]:
            return "invalid_conv"
        if kind == "reframe" and (v[2], v[3]) != (c["ow"], c["oh"]):
            return "invalid_reframe"
        if kind == "deint" and v == DEINT_FIELD and c["F"] % 2:
            return "field_F"
        if kind == "ivtc" and (c["F"] < 4 or c["F"] % 4):
            return "ivtc_F"
    if q["busy"]:
        return "busy"
    if kind == "deint" and v is not None and c["temporal"] == ("ivtc",):
        return "deint_while_ivtc"
    if kind == "ivtc" and v is not None and c["temporal"] and c["temporal"][0] == "deint":
        return "ivtc_while_deint"
    if kind == "reframe" and front:
        return "reframe_while_front"
    if kind == "reframe" and c["orient"]:
        return "reframe_while_orient"
    if kind == "orient" and front:
        return "orient_while_front"
    return None


def plan_set(c, q):
    """-> dict(rc, reason, noop, next, geom (of next), alloc[7], free[7], reset[7])"""
    o = dict(rc=0, reason=None, noop=False, next=dict(c, ov_clip=list(c["ov_clip"])), geom=geometry(c), alloc=[0] * 7, free=[False] * 7, reset=[False] * 7)
    o["reason"] = refusal(c, q)
    if o["reason"]:
        o["rc"] = ERR_ARG
        return o
    kind, pos = q["kind"], POS[q["kind"]]
    if q["op"] == "reset":
        o["reset"][pos] = True
    if q["op"] != "set":
        return o
    v = q["value"]
    if kind in ("levels", "reframe") and q.get("identity"):
        v = None
    if kind == "orient" and v == 0:
        v = None
    slot = ORDER[pos]
    if pos == 2 and c["temporal"] and c["temporal"][0] != kind:
        o["noop"] = True                # clearing the one that is not set while the other one is: OK, untouched
        return o
    if v is None and not is_set(c, slot):
        o["noop"] = True
        # open: clearing a deinterlacer that is not set forgets the noise filter's state, the inverse telecine's twin does not
        if kind == "deint" and c["denoise"]:
            o["reset"][3] = True
        return o
    n = o["next"]
    if kind == "conv":
        n["conv"] = None if v is None else (v[0], v[1])
    elif kind == "deint":
        n["temporal"] = None if v is None else ("deint", v)
    elif kind == "ivtc":
        n["temporal"] = None if v is None else ("ivtc",)
    elif kind == "orient":
        n["orient"] = v or 0
    elif kind == "reframe":
        n["reframe"] = None if v is None else (v[0], v[1])
    else:
        n[slot] = v is not None
    g = o["geom"] = geometry(n)
    if kind == "overlays":
        o["reset"][6] = v is not None           # a list's counters start at 0
        if v is None:                           # the pass's own clips go with the list
            o["free"][6] = any(c["ov_clip"])
            n["ov_clip"] = [False, False]
        return o
    o["free"][pos] = is_set(c, slot)
    o["alloc"][pos] = clip_bytes(n, g, pos) if v is not None else 0
    if kind == "ivtc" and g["conv_frames"] != geometry(c)["conv_frames"]:
        for p, s in ((0, "conv"), (1, "levels")):           # what a call brings changed: re-sized in the same step
            if is_set(c, s):
                o["free"][p], o["alloc"][p] = True, clip_bytes(n, g, p)
    if kind == "levels":
        o["reset"][2] = is_set(c, "temporal")
    if kind in ("levels", "deint", "ivtc"):
        o["reset"][3] = c["denoise"]
    return o


CALLER, UPLOAD = -1, -2
KIND_AT = {0: "conv", 1: "levels", 3: "denoise", 4: "orient", 5: "reframe"}


def plan_call(c, form, active, par):
    """one call: form 0 host / 1 plain device / 2 held.  -> dict(rc, bypass, upload, steps [(kind, nframes, src, dst, bytes, alloc)],
    out, advance); kind "copy": the device-to-device copy into the overlay pass's clip"""
    g = geometry(c)
    o = dict(rc=0, bypass=False, upload=0, steps=[], out=CALLER, advance=0)
    if not g["lane"]:
        o["rc"] = ERR_ARG
        return o
    o["advance"] = c["F"] if c["overlays"] else 0
    blend = c["overlays"] and active
    writes = any(is_set(c, s) for s in ORDER[:6])
    if not blend and not writes and (form or not c["keep_lane"]):
        o["bypass"] = True
        return o
    cur = CALLER
    if not form:
        o["upload"], cur = g["bytes_in"], UPLOAD
    for pos in range(6):
        if not is_set(c, ORDER[pos]):
            continue
        kind = c["temporal"][0] if pos == 2 else KIND_AT[pos]
        n = c["nsrc"] * g["frames_in"] if pos <= 1 else g["frames_in"] if pos == 2 else c["F"] if pos == 3 else c["nsrc"] * c["F"]
        o["steps"].append((kind, n, cur, pos, 0, 0))
        cur = pos
    if blend:
        if cur == CALLER:                       # a caller's device clip is never written
            b = clip_bytes(c, g, 6)
            o["steps"].append(("copy", c["nsrc"] * c["F"], cur, 6, b, 0 if c["ov_clip"][par] else b))
            cur = 6
        o["steps"].append(("overlays", c["F"], cur, cur, 0, 0))
    o["out"] = cur
    return o
