"""The two plans of a packet fetch (csrc/dsvg_fetch_plan.h: plan_fetch_wait, plan_fetch_layout), asked through the device-free query
dsvg_fetch_plan, against the restatement of tests/fetch_plan.py over a seeded sweep, with the invariants of the layout and the cases
the design pins."""
import functools
import importlib
import itertools
import random

import pytest

import fetch_plan as F

K = 65536


@functools.lru_cache(maxsize=None)
def package():
    return importlib.import_module("digital-subband-video-1_amd")


GEOS = (F.bits_geo(96, 64, 48, 32), F.bits_geo(256, 256, 128, 128))          # luma capacity 12 288 (below the round trip's 64 KB) and 131 072 (above)


def ask(a):
    return package().fetch_plan(a["O"], a["slots"], a["ev"], a["isP"], a["ring"], a["ncalls"], a["cb"], package().FETCH_NO_FAST if a["no_fast"] else 0,
                                a["per_job"], a["off"], a["cap"], a["bits"], a["ov"], a["nchunks"], a["align"])


def want(a):
    return F.plan(a["O"], a["slots"], a["ev"], a["isP"], a["ring"], a["ncalls"], a["cb"], a["no_fast"], a["per_job"], a["off"], a["cap"], a["bits"],
                  a["ov"], a["nchunks"], a["align"])


def check(a):
    """the query against the restatement, then the invariants; -> the query's plan, or the refusal"""
    try:
        w = want(a)
    except F.Refused as e:
        with pytest.raises(package().FetchRefused) as r:
            ask(a)
        assert (r.value.rc, r.value.text) == (e.rc, e.text), a
        # a refusal reports no growth (an overflow found behind the one round trip: that path's fixed pair was taken before)
        assert r.value.grow == 0 and r.value.grow_few == getattr(e, "grow_few", 0), a
        e.grow_few = r.value.grow_few
        return e
    g = ask(a)
    n = len(a["slots"])
    for k in ("few", "stream_wait", "wait", "lo", "hi", "grow_few", "fits", "general", "total", "grow", "nchunks", "pieces"):
        assert g[k] == w[k], (k, g[k], w[k], a)
    for k in ("copies", "rows", "nbytes", "pay"):
        assert g[k].tolist() == [[list(r) if isinstance(r, tuple) else r for r in pic] for pic in w[k]], (k, a)
    assert len(set(g["wait"])) == len(g["wait"]) and -1 not in g["wait"] and all(0 <= e < a["ring"] for e in g["wait"])
    assert g["stream_wait"] == g["few"] and (g["grow_few"] == 12 * K + 64) == bool(g["few"])
    if g["few"]:
        assert all(c[1] + c[2] <= 12 * K for pic in g["copies"] for c in pic.tolist())
    if not g["general"]:
        assert g["grow"] == 0 and not g["pieces"] and all(b <= K for b in g["nbytes"].reshape(-1).tolist())
        return g
    dst = [r[1] for pic in g["rows"].tolist() for r in pic]
    end = [r[1] + r[2] for pic in g["rows"].tolist() for r in pic]
    assert all(d % 16 == 0 for d in dst) and dst[0] == 0
    assert all(e <= d2 for e, d2 in zip(end, dst[1:])) and dst == sorted(dst) and end[-1] <= g["total"] and g["total"] % 16 == 0
    assert g["grow"] == g["total"] + 64
    p = g["pieces"]
    assert p[0][0] == 0 and p[-1][1] == n and all(x[1] == y[0] for x, y in zip(p, p[1:])) and all(x[0] < x[1] for x in p)
    assert all(x[1] % a["align"] == 0 for x in p[:-1])
    assert p[0][2] == 0 and p[-1][3] == g["total"] and all(x[3] == y[2] for x, y in zip(p, p[1:])) and all(x[2] <= x[3] for x in p)
    assert len(p) == g["nchunks"] <= (a["nchunks"] if a["cb"] else 1)
    return g


def slot_events(kind, O, ring, ncalls, rng):
    newest = (ncalls - 1) % ring
    if kind == "newest":
        return [newest] * O
    if kind == "holes":
        return [-1 if rng.random() < 0.4 else newest for _ in range(O)]
    return [rng.choice([-1] + list(range(ring))) for _ in range(O)]


def is_p(kind, O, rng):
    if kind == "empty":
        return []
    full = [1] * O if kind.endswith("P") else [int(rng.random() < 0.7) for _ in range(O)]
    return full[:max(O // 2, 1)] if kind.startswith("short") else full


def plane_bits(cap, rng, seen):
    pick = rng.choice(["empty", "K", "K+1", "cap", "small", "small", "small", "small"])
    b = {"empty": 0, "K": K * 8 - rng.randrange(8), "K+1": K * 8 + 1 + rng.randrange(8), "cap": cap * 8}.get(pick, rng.randrange(1, 3000 * 8))
    if b > cap * 8:                                    # (a plane of a small geometry: nothing beyond its capacity)
        pick, b = "small", rng.randrange(1, 3000 * 8)
    seen.add(pick)
    return b


def test_the_query_is_the_restatement_over_the_sweep():
    rng = random.Random(0xFE7C)
    rest = list(itertools.product((False, True), (False, True), (1, 4, 7), (1, 2, 3, "n+2")))        # callback, switch, nchunks, align
    seen, paths, k = set(), {"few": 0, "fell": 0, "general": 0, "refused": 0, "overflow": 0}, 0
    for n, O, ring, evk, pk in itertools.product(range(1, 10), (1, 4, 12, 48), (4, 10), ("newest", "holes", "mixed"),
                                                  ("empty", "shortP", "short", "fullP", "full")):
        for _ in range(4):
            cb, no_fast, nchunks, align = rest[k % len(rest)]
            per_job, off, cap = GEOS[(k // len(rest)) % 2]
            k += 1
            ncalls = rng.randrange(1, 40)
            slots = [rng.randrange(O) for _ in range(n)] if rng.random() < 0.5 or n > O else rng.sample(range(O), n)
            a = dict(O=O, slots=slots, ev=slot_events(evk, O, ring, ncalls, rng), isP=is_p(pk, O, rng), ring=ring, ncalls=ncalls, cb=cb, no_fast=no_fast,
                     per_job=per_job, off=off, cap=cap, bits=[[plane_bits(cap[p], rng, seen) for p in range(3)] for _ in range(n)],
                     ov=[[int(rng.random() < 0.01) for _ in range(3)] for _ in range(n)], nchunks=nchunks, align=n + 2 if align == "n+2" else align)
            g = check(a)
            if isinstance(g, F.Refused):
                paths["overflow" if g.rc == F.ERR_OVERFLOW else "refused"] += 1
                assert (n > O) == (g.rc == F.ERR_ARG)
            else:
                paths["few" if g["fits"] else "fell" if g["few"] else "general"] += 1
    assert k == 9 * 4 * 2 * 3 * 5 * 4 and seen == {"empty", "K", "K+1", "cap", "small"}
    assert all(v > 50 for v in paths.values()), paths


def base(**kw):
    per_job, off, cap = GEOS[1]
    a = dict(O=12, slots=[0, 1, 2, 3], ev=[2] * 12, isP=[1] * 12, ring=4, ncalls=7, cb=False, no_fast=False, per_job=per_job, off=off, cap=cap,
             bits=None, ov=None, nchunks=1, align=1)
    a.update(kw)
    n = len(a["slots"])
    a["bits"] = a["bits"] or [[8 * 100] * 3] * n
    a["ov"] = a["ov"] or [[0] * 3] * n
    return a


def test_pinned_paths():
    g = check(base())
    assert g["few"] and g["fits"] and not g["general"] and g["wait"] == [2] and g["stream_wait"]
    assert g["pay"].tolist() == [[(3 * i + p) * K for p in range(3)] for i in range(4)]
    assert not check(base(slots=[0, 1, 2, 3, 4]))["few"]                                 # n = 5
    isP = [1] * 12
    isP[2] = 0
    g = check(base(isP=isP))                                                             # n = 4 with one I picture
    assert not g["few"] and g["general"] and not g["stream_wait"] and g["grow_few"] == 0
    assert not check(base(cb=True))["few"]                                               # all P, newest call, but a callback
    assert not check(base(no_fast=True))["few"]
    assert not check(base(ev=[2, 2, 1, 2] + [2] * 8))["few"]                             # a slot of an older call
    g = check(base(ev=[-1] * 12, isP=[], ncalls=0, bits=[[0] * 3] * 4))                  # a bare context
    assert g["few"] and g["fits"] and g["wait"] == [] and g["grow_few"] == 12 * K + 64
    assert check(base(isP=[1]))["few"]                                                   # a short table: the slots beyond it count as P


def test_pinned_fall_through_and_sizes():
    cap = GEOS[1][2]
    g = check(base(slots=[5], bits=[[8 * K, 0, 8 * 100]]))                               # exactly 64 KB: the round trip holds it
    assert g["few"] and g["fits"] and g["nbytes"].tolist() == [[K, 0, 100]]
    g = check(base(slots=[5], bits=[[8 * K + 1, 0, 8 * 100]]))                           # one bit more: the general path behind the round trip
    assert g["few"] and not g["fits"] and g["general"] and g["stream_wait"] and g["grow_few"] == 12 * K + 64
    assert g["nbytes"].tolist() == [[K + 1, 0, 100]] and g["total"] == K + 16 + 112 and g["grow"] == g["total"] + 64
    assert g["rows"].tolist() == [[[5 * GEOS[1][0], 0, K + 1], [5 * GEOS[1][0] + GEOS[1][1][1], K + 16, 0], [5 * GEOS[1][0] + GEOS[1][1][2], K + 16, 100]]]
    assert g["pieces"] == [(0, 1, 0, g["total"])] and (g["lo"], g["hi"]) == (5, 5)
    g = check(base(slots=[5], bits=[[8 * cap[0], 8 * cap[1], 0]]))                       # planes at their capacity
    assert g["general"] and g["nbytes"].tolist() == [[cap[0], cap[1], 0]]
    per_job, off, small = GEOS[0]
    g = check(base(slots=[1], per_job=per_job, off=off, cap=small, bits=[[8 * small[0], 0, 0]]))
    assert g["fits"] and g["copies"][0].tolist() == [[per_job + off[p], p * K, small[p]] for p in range(3)]


def test_pinned_pieces_of_the_headline():
    """what dsv1_batch_collect asks for at the headline: 16 streams x 12 frames, four pieces that end on whole streams"""
    S, nf = 16, 12
    n = S * nf
    g = check(base(O=2 * n, slots=list(range(n)), ev=[0] * (2 * n), isP=[1] * (2 * n), cb=True, nchunks=4, align=nf, bits=[[8 * 100, 8 * 33, 3]] * n))
    pic = 112 + 48 + 16
    assert g["pieces"] == [(0, 48, 0, 48 * pic), (48, 96, 48 * pic, 96 * pic), (96, 144, 96 * pic, 144 * pic), (144, 192, 144 * pic, 192 * pic)]
    assert g["total"] == n * pic and not g["stream_wait"] and g["wait"] == [0]
    # fewer whole groups than pieces asked for; a group larger than the call; no callback: one piece
    assert [x[:2] for x in check(base(slots=list(range(7)), cb=True, nchunks=4, align=3))["pieces"]] == [(0, 3), (3, 7)]
    assert [x[:2] for x in check(base(slots=list(range(7)), cb=True, nchunks=7, align=1))["pieces"]] == [(i, i + 1) for i in range(7)]
    assert [x[:2] for x in check(base(slots=list(range(7)), cb=True, nchunks=4, align=9))["pieces"]] == [(0, 7)]
    assert [x[:2] for x in check(base(slots=list(range(7)), cb=False, nchunks=4, align=1))["pieces"]] == [(0, 7)]
    assert [x[:2] for x in check(base(slots=list(range(9)), cb=True, nchunks=4, align=2))["pieces"]] == [(0, 2), (2, 4), (4, 6), (6, 9)]


def test_wait_list_order():
    g = check(base(slots=[3, 0, 1, 2, 0], ev=[1, 3, -1, 3] + [0] * 8))
    assert g["wait"] == [3, 1] and not g["stream_wait"]


@pytest.mark.parametrize("kw,rc,text", [
    (dict(slots=[]), -2, "bad fetch_pictures arguments"), (dict(nchunks=0), -2, "bad fetch_pictures arguments"),
    (dict(align=0), -2, "bad fetch_pictures arguments"), (dict(O=3), -2, "bad fetch_pictures arguments"),
    (dict(slots=[0, 12]), -2, "out slot out of range"), (dict(slots=[-1]), -2, "out slot out of range"),
    (dict(slots=[4, 7], ov=[[0, 0, 0], [0, 1, 1]]), -4, "packed plane 1 of out slot 7 exceeds 32768 bytes"),
    (dict(slots=[4, 7], cb=True, ov=[[0, 0, 1], [1, 0, 0]]), -4, "packed plane 2 of out slot 4 exceeds 32768 bytes"),
])
def test_refusals(kw, rc, text):
    e = check(base(**kw))
    assert isinstance(e, F.Refused) and (e.rc, e.text) == (rc, text)
    assert e.grow_few == (12 * K + 64 if rc == -4 and not kw.get("cb") else 0)
