"""CPU checks of the plan of a coding call (csrc/dsvg_batch_plan.h: plan_code_batch, which dsvg_code_batch commits and enqueues from),
asked through the device-free query dsvg_code_batch_plan on the calls of tests/batch_cases.py.

Every property is checked against a definition written out here from the call as the caller states it -- never against another value
of the plan than the one the definition is about (the group split gk and the I counts nI are checked first, by their own definitions,
and then used).  The library is loaded; no device is needed."""
import functools

import numpy as np
import pytest

import batch_cases as K

BORDER = 64
ERR_ARG = -2


@functools.lru_cache(maxsize=None)
def cases():
    """(scenario, plan) of every call of the matrix, planned once"""
    return tuple((sc, sc.plan()) for sc in K.scenarios())


def device_order(sc, t):
    """caller indices of step t in device order: the stable partition, I pictures first"""
    js = [sc.job(t, i) for i in range(sc.njobs)]
    return [i for i, j in enumerate(js) if j["ref"] < 0] + [i for i, j in enumerate(js) if j["ref"] >= 0]


def device_jobs(sc):
    """the jobs of the call in device order, step after step"""
    return [sc.job(t, i) for t in range(sc.nsteps) for i in device_order(sc, t)]


def group_of(gk, k):
    return max(g for g in range(len(gk) - 1) if gk[g] <= k)


def test_matrix_is_what_the_families_say():
    names = [sc.name for sc, _ in cases()]
    assert len(set(names)) == len(names)
    for geom in K.GEOMS:
        for S in K.STREAMS:
            for T in K.STEPS:
                assert "%s/a/S%dT%d" % (geom, S, T) in names
    fused = {sc.geom: p["mc_fused"] for sc, p in cases()}
    assert fused["96x64"] == 1 and fused["384x240"] == 0 and fused["1080p"] == 1
    assert {sc.geom: p["nblk"] for sc, p in cases()}["1080p"] == 690
    for sc, p in cases():
        assert p["nblk"] == sc.nblk and p["total"] == sc.total and p["base"] == min(j["out"] for j in sc.jobs)


def test_order_is_the_stable_partition():
    for sc, p in cases():
        for t in range(sc.nsteps):
            want = device_order(sc, t)
            assert list(p["order"][t * sc.njobs:(t + 1) * sc.njobs]) == want, sc.name
            assert p["nI"][t] == sum(sc.job(t, i)["ref"] < 0 for i in range(sc.njobs)), sc.name


def test_groups_split_the_positions_evenly():
    for sc, p in cases():
        assert 1 <= p["ng"] <= 4 and p["gk"] == tuple(sc.njobs * g // p["ng"] for g in range(p["ng"] + 1)), sc.name


def replay_is_safe(sc, gk):
    """no reconstruction slot is read or written by another group than the one that wrote it last in an earlier step of the call, and no
    slot is written by two groups in one step"""
    last = {}
    for t in range(sc.nsteps):
        now = {}
        for k, i in enumerate(device_order(sc, t)):
            j, g = sc.job(t, i), group_of(gk, k)
            if j["ref"] >= 0 and last.get(j["ref"], g) != g:
                return False
            if j["recon"] >= 0:
                if last.get(j["recon"], g) != g or now.get(j["recon"], g) != g:
                    return False
                now[j["recon"]] = g
        last.update(now)
    return True


def test_two_groups_never_share_a_slot():
    split = 0
    for sc, p in cases():
        if p["ng"] > 1:
            split += 1
            assert replay_is_safe(sc, p["gk"]), sc.name
    assert split > 50


def test_the_replay_sees_a_shared_slot():
    """(the definition above is not vacuous: the reversed call, split by force, fails it)"""
    sc = K.build("96x64", "b", 16, 2, seed=1)
    assert not replay_is_safe(sc, (0, 8, 16))
    assert replay_is_safe(K.build("96x64", "a", 16, 2), (0, 8, 16))


def test_liveness_of_the_split():
    """a wrong fallback to one stream passes every byte comparison and loses the speed"""
    P = K.pkg()
    seen = set()
    for sc, p in cases():
        fam = sc.name.split("/")[1]
        if fam == "a":
            S = sc.S
            if S >= 2:
                assert p["ng"] == 2, sc.name
                assert sc.plan(P.BATCH_NO_SMALL_SPLIT)["ng"] == (1 if S < 16 else 2), sc.name
            else:
                assert p["ng"] == 1, sc.name
            assert sc.plan(code_streams=1)["ng"] == 1, sc.name
            seen.add(("a", S >= 16))
        if fam == "b" and "seed" not in sc.name and sc.S == 16:             # (seed 1: the odd steps reversed)
            assert p["ng"] == 1, sc.name
            seen.add("b")
        if fam in ("c", "d"):
            assert p["ng"] == 1, sc.name
            seen.add(fam)
        if fam in ("e", "f", "g") and sc.njobs >= 2:
            assert p["ng"] == 2, sc.name                   # (streams at their positions, own slots: nothing to fall back for)
    assert seen == {("a", False), ("a", True), "b", "c", "d"}


def per_block_need(sc, mv):
    """how far a picture with the vectors `mv` reads beyond the edges of its reference, block by block: luma [0..3] and chroma [4..7]
    pixels left, right, above, below.  The window of an inter block starts at the clamped position of bmc.c:248-255 and is read with a
    margin of 2 pixels before and 3 after; a reference that is read at all is read 16 columns / 8 rows out; a need above BORDER - 4 on
    any side means the whole border on every side."""
    need = np.array([16, 16, 8, 8, 16, 16, 8, 8])
    inter = mv["mode"] == 0
    b = np.arange(sc.nblk)
    for pl in range(2):
        sh, sv = (sc.hs, sc.vs) if pl else (0, 0)
        bw, bh = sc.bw >> sh, sc.bh >> sv
        pw, ph = (-(-sc.w // (1 << sh)), -(-sc.h // (1 << sv))) if pl else (sc.w, sc.h)
        x, y = (b % sc.nbh) * bw, (b // sc.nbh) * bh
        on = inter & (x < pw) & (y < ph)
        if not on.any():
            continue
        x, y = x[on], y[on]
        cw, ch = np.minimum(bw, pw - x), np.minimum(bh, ph - y)
        dx, dy = mv["x"][on].astype(np.int64) >> sh, mv["y"][on].astype(np.int64) >> sv
        wx = np.clip(x + (dx >> 1), -BORDER, pw - bw + BORDER - 1)
        wy = np.clip(y + (dy >> 1), -BORDER, ph - bh + BORDER - 1)
        n = np.array([(2 - wx).max(), (wx + cw + 3 - (pw - 1)).max(), (2 - wy).max(), (wy + ch + 3 - (ph - 1)).max()])
        need[4 * pl:4 * pl + 4] = np.maximum(need[4 * pl:4 * pl + 4], n)
    return np.full(8, BORDER) if (need > BORDER - 4).any() else need


def border_extents(sc, lazy=True):
    """ext[d] of every device job, and whether a reader with has_reach contributed to it.  A reconstruction gets the most that any
    picture predicting from it needs until its slot is written again (the pictures of the step that rewrites it still read the old
    one); a job that keeps none gets 0; the last writer of a slot gets the whole border unless border_hint vouches for it."""
    dj = device_jobs(sc)
    ext = np.zeros((sc.total, 8), dtype=np.int64)
    summarised = np.zeros(sc.total, dtype=bool)
    if not lazy:
        return ext + BORDER, summarised
    need = {}
    writer = {}
    for t in range(sc.nsteps):
        step = range(t * sc.njobs, (t + 1) * sc.njobs)
        for d in step:
            j = dj[d]
            w = writer.get(j["ref"]) if j["ref"] >= 0 else None
            if w is not None:
                if j["mv"] not in need:
                    need[j["mv"]] = per_block_need(sc, sc.mv_tables[j["mv"]])
                ext[w] = np.maximum(ext[w], need[j["mv"]])
                summarised[w] |= bool(j["has_reach"])
        for d in step:
            if dj[d]["recon"] >= 0:
                writer[dj[d]["recon"]] = d
    for d in writer.values():
        if not dj[d]["hint"]:
            ext[d] = BORDER
            summarised[d] = False
    return ext, summarised


def test_border_extents():
    P = K.pkg()
    exact = above = 0
    for sc, p in cases():
        want, summarised = border_extents(sc)
        got = p["ext"].astype(np.int64)
        assert got.shape == want.shape
        assert (got[~summarised] == want[~summarised]).all(), sc.name
        assert (got[summarised] >= want[summarised]).all() and (got[summarised] <= BORDER).all(), sc.name
        exact += int((~summarised).sum())
        above += int((got[summarised] > want[summarised]).any(axis=1).sum())
    assert exact > 1000 and above > 0
    for sc, p in cases()[:40]:
        off = sc.plan(P.BATCH_NO_LAZY_BORDER)["ext"]
        assert (off == BORDER).all(), sc.name


def test_border_extents_take_every_value():
    """(the matrix reaches extents that are 0, the minimum of a referenced picture, in between, and the whole border)"""
    vals = set()
    for sc, p in cases():
        vals |= set(np.unique(p["ext"][:, :4]).tolist())
    assert {0, 16, BORDER} <= vals and any(16 < v < BORDER - 4 for v in vals) and not any(BORDER - 4 < v < BORDER for v in vals)


def test_shared_tables():
    shared = 0
    for sc, p in cases():
        dj = device_jobs(sc)
        n = sc.total
        for key, idx, cp, cnt in (("st", p["stu"], p["stcp"], p["nst"]), ("mv", p["mvu"], p["mvcp"], p["nmv"])):
            assert sorted(set(idx.tolist())) == list(range(cnt)), sc.name
            by_index = {}
            for d in range(n):
                by_index.setdefault(int(idx[d]), []).append(d)
            for u, ds in by_index.items():
                tabs = {dj[d][key] for d in ds}
                if key == "mv" and None in tabs:
                    assert len(ds) == 1 and dj[ds[0]]["ref"] < 0 and not cp[ds[0]], sc.name     # an I picture: an index of its own, nothing copied
                    continue
                assert len(tabs) == 1, sc.name                                           # one index: one pointer
                marked = [d for d in ds if cp[d]]
                assert len(marked) == 1, sc.name
                if key == "mv":
                    assert dj[marked[0]]["ref"] >= 0, sc.name
                shared += len(ds) > 1
            tab_index = {}
            for d in range(n):                                                           # one pointer: one index
                if dj[d][key] is not None:
                    assert tab_index.setdefault(dj[d][key], int(idx[d])) == int(idx[d]), sc.name
        assert p["mv_contig"] == (p["nmv"] == n), sc.name
    assert shared > 20


def test_intra_lists():
    listed = empty = 0
    for sc, p in cases():
        dj = device_jobs(sc)
        ng, gk = p["ng"], p["gk"]
        want_all = []
        for t in range(sc.nsteps):
            nI = sum(sc.job(t, i)["ref"] < 0 for i in range(sc.njobs))
            for g in range(ng):
                want, anyP = [], False
                for k in range(gk[g], gk[g + 1]):
                    j = dj[t * sc.njobs + k]
                    if j["ref"] < 0:
                        continue
                    anyP = True
                    if p["mc_fused"] and not j["no_intra"]:
                        blocks = np.flatnonzero(sc.mv_tables[j["mv"]]["mode"] != 0)
                        want += ((k - max(gk[g], nI)) * sc.nblk + blocks).tolist()
                got = p["ilist"][p["ioff"][t, g]:p["ioff"][t, g] + p["icnt"][t, g]].tolist()
                assert got == want, (sc.name, t, g)
                assert p["noint"][t, g] == (0 if (not p["mc_fused"] and anyP) else 1), (sc.name, t, g)
                want_all += want
                listed += len(want) > 0
                empty += anyP and not want
        assert p["iln"] == len(want_all) and p["ilist"].tolist() == want_all, sc.name
    assert listed > 100 and empty > 100


def test_rate_control_chain():
    n = 0
    for sc, p in cases():
        if sc.rc is None:
            assert (p["rc_next"] == -1).all(), sc.name
            continue
        n += 1
        pos = [{i: k for k, i in enumerate(device_order(sc, t))} for t in range(sc.nsteps)]
        for t in range(sc.nsteps):
            for i in range(sc.njobs):
                want = p["base"] + (t + 1) * sc.njobs + pos[t + 1][i] if t + 1 < sc.nsteps else -1
                assert p["rc_next"][t * sc.njobs + pos[t][i]] == want, (sc.name, t, i)
    assert n >= 7 * len(K.GEOMS)


def test_keeps_and_par_enqueue():
    P = K.pkg()
    par = 0
    for sc, p in cases():
        dj = device_jobs(sc)
        for t in range(sc.nsteps):
            for g in range(p["ng"]):
                want = any(dj[t * sc.njobs + k]["recon"] >= 0 for k in range(p["gk"][g], p["gk"][g + 1]))
                assert p["keeps"][t, g] == want, (sc.name, t, g)
        want = p["ng"] > 1 and sc.nsteps * 13 >= 100 and sc.njobs < 64
        assert p["par_enqueue"] == want, sc.name
        if want:
            par += 1
            assert not sc.plan(P.BATCH_PROFILED)["par_enqueue"] and not sc.plan(P.BATCH_NO_PAR_ENQUEUE)["par_enqueue"], sc.name
    assert par > 20


def refused(sc, **kw):
    with pytest.raises(K.pkg().BatchRefused) as e:
        sc.plan(**kw)
    return e.value.rc, e.value.text


def test_refusals():
    """every argument error of the call: its code and its text, in the order the call checks"""
    def call(rc=False):
        return K.build("96x64", "c", 4, 3, rc=rc)       # step 1 or 2 is mixed: device order differs from the caller's
    sc = call()
    sc.max_jobs = 3
    assert refused(sc) == (ERR_ARG, "bad code_batch arguments")
    sc = call()
    sc.out_slots = 11
    assert refused(sc) == (ERR_ARG, "bad code_batch arguments")
    for n in ((0, 4), (3, 0), (-1, 4)):
        sc = call()
        sc.nsteps, sc.njobs = n
        assert refused(sc) == (ERR_ARG, "bad code_batch arguments")
    sc = call()
    for j in sc.jobs:
        j["out"] += 4                                    # the block ends behind the context's out slots
    assert refused(sc) == (ERR_ARG, "out slots of a batch must be a contiguous block")
    sc = call()
    sc.jobs[5]["out"] = -1
    assert refused(sc) == (ERR_ARG, "out slots of a batch must be a contiguous block")
    sc = call()
    sc.jobs[6]["out"] = 14                               # a hole in the block: 12 pictures from slot 0, one of them at 14
    assert refused(sc) == (ERR_ARG, "bad picture job (step 1 job 2)")
    for field, bad in (("src", -1), ("src", sc.n_src), ("recon", sc.n_recon), ("ref", sc.n_recon), ("st", None)):
        sc = call()
        sc.jobs[4 + 1][field] = bad
        if field == "ref":
            sc.jobs[5]["mv"] = sc.jobs[5]["mv"] if sc.jobs[5]["mv"] is not None else 0
        assert refused(sc) == (ERR_ARG, "bad picture job (step 1 job 1)"), field
    sc = call()
    t, i = next((t, i) for t in (1, 2) for i in range(4) if sc.job(t, i)["ref"] >= 0)
    sc.job(t, i)["mv"] = None                            # a P picture without vectors
    assert refused(sc) == (ERR_ARG, "bad picture job (step %d job %d)" % (t, i))
    # device order: of two bad jobs of a step the I picture is found first, whatever its place
    sc = call()
    t = next(t for t in (1, 2) if any(sc.job(t, i)["ref"] < 0 for i in range(4)))
    iI = next(i for i in range(4) if sc.job(t, i)["ref"] < 0)
    iP = next(i for i in range(4) if sc.job(t, i)["ref"] >= 0)
    sc.job(t, iI)["src"] = sc.job(t, iP)["src"] = -1
    assert refused(sc) == (ERR_ARG, "bad picture job (step %d job %d)" % (t, iI))
    # rate control
    sc = call(rc=True)
    sc.rc[5] = (max(sc.n_recon, sc.max_jobs), 0, 0)
    assert refused(sc) == (ERR_ARG, "bad rate-control job 5")
    sc = call(rc=True)
    sc.rc[2] = (2, -1, 0)
    assert refused(sc) == (ERR_ARG, "bad rate-control job 2")
    sc = call(rc=True)
    sc.rc[6] = (7, 0, 0)
    assert refused(sc) == (ERR_ARG, "a stream must keep its position from frame step to frame step (rate-control job 6)")
    sc = call(rc=True)
    sc.rc[3] = (1, 0, 0)
    assert refused(sc) == (ERR_ARG, "two pictures of one rate-controlled stream in one frame step (jobs 1, 3)")
    # the order of the checks: call arguments, rate control, the out-slot block, the pictures
    sc = call(rc=True)
    sc.rc[3] = (1, 0, 0)
    sc.jobs[5]["out"] = -1
    sc.jobs[0]["src"] = -1
    assert refused(sc)[1].startswith("two pictures")
    sc.rc[3] = (3, 0, 0)
    assert refused(sc)[1].startswith("out slots")
    sc.jobs[5]["out"] = 5
    assert refused(sc)[1] == "bad picture job (step 0 job 0)"
    sc.max_jobs = 3
    assert refused(sc)[1] == "bad code_batch arguments"


def test_query_refuses_what_the_context_refuses():
    sc = K.build("96x64", "a", 2, 2)
    sc.w = 31
    assert refused(sc)[0] == ERR_ARG
    sc = K.build("96x64", "a", 2, 2)
    sc.h = 65
    assert refused(sc)[0] == -3
