"""The decisions of an encoder session's submit (csrc/host/dsv1_submit_plan.h through dsv1_submit_plan, no device) against their
restatement (tests/submit_plan.py), over seeded sequences of 1 to 4 calls that carry the state from call to call; the invariants of
the job tables over every sequence; and that the cases reach every class of decision."""
import collections
import importlib
import random

import pytest

import submit_plan as SP

NBLK, THRESH, NPIX = 20, 50, 12
SRC_FIELDS = ("next_fnum", "prev_gop", "gop", "force_metadata", "do_scd", "prev_avg_luma", "scene_change_delta")
PIC_FIELDS = ("fnum", "gop_start", "is_ref", "has_ref", "forced_intra", "isP", "n_intra", "cur_slot", "ref_slot", "out_slot")
MODES = ("crf", "devabr", "serial")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("digital-subband-video-1_amd")
    p.lib()
    return p


def sequences():
    """(seed, S, R, F, gop, mode, chains, keep_all, do_scd, ncalls): every S, R, F, gop and chains of the issue's lists occurs"""
    out = []
    for seed in range(420):
        rnd = random.Random(0x5B17 + seed)
        chains = rnd.choice((0, 0, 1, 2, 4))
        S, R = (1, 1) if chains else (rnd.choice((1, 2, 3)), rnd.choice((1, 3)))
        mode = "crf" if chains else rnd.choice(MODES)
        out.append((seed, S, R, rnd.choice((1, 3, 4, 6, 12)), rnd.choice((0, 1, 4, 6, 12)), mode, chains, rnd.random() < 0.2,
                    rnd.random() < 0.7, rnd.randint(1, 4)))
    return out


def run_sequence(pkg, case, seen, counts):
    seed, S, R, F, gop, mode, chains, keep_all, do_scd, ncalls = case
    rnd = random.Random(seed)
    N, rows = S * R, 2 * F + 1
    abr, serial = mode != "crf", mode == "serial"
    srcs = [dict(next_fnum=rnd.choice((0, 0, 5, 0xFFFFFFFE)), prev_gop=0xFFFFFFFF, gop=gop, force_metadata=1, do_scd=int(do_scd),
                 prev_avg_luma=0, scene_change_delta=4) for _ in range(S)]
    streams = [dict(cur=k, has_recon=0, border_skipped=0, recon_dropped=0) for k in range(N)]
    c_src = [pkg.SubmitSrc(*[d[f] for f in SRC_FIELDS]) for d in srcs]
    c_st = [pkg.SubmitStream() for _ in range(N)]
    luma = [0] * (rows * S)
    level = [rnd.randint(60, 180) for _ in range(S)]
    carry, gcount, par, nf_prev = [-1, -1], 0, 0, 0
    prev_model, prev_lib = None, None
    writer, coded = {}, [0] * N                              # invariant 1: slot -> (stream, running picture number)
    for call in range(ncalls):
        nf = rnd.randint(1, F) if (N == 1 and call == ncalls - 1 and rnd.random() < 0.5) else F
        for s in range(S):
            for t in range(nf):
                if rnd.random() < 0.12:
                    level[s] = rnd.randint(20, 230)         # a scene cut (or not, when it lands near the old level)
                luma[((gcount + t) % rows) * S + s] = (level[s] + rnd.randint(0, 2)) * NPIX + rnd.randint(0, NPIX - 1)
        n_intra = [rnd.randint(11, NBLK) if rnd.random() < 0.15 else rnd.randint(0, 5) for _ in range(N * F)]
        g = dict(S=S, R=R, F=F, nf=nf, chains=chains, gcount=gcount, par=par, npix_small=NPIX, nblk=NBLK, intra_pct_thresh=THRESH,
                 abr=int(abr), serial=int(serial), keep_all=int(keep_all), nf_prev=nf_prev, carry=list(carry))
        q = pkg.SubmitQuery(S, R, F, nf, chains, gcount, par, NPIX, NBLK, THRESH, int(abr), int(serial), int(keep_all), nf_prev,
                            (pkg._C.c_int * 2)(*carry))
        before = [dict(d) for d in streams]
        want = SP.plan(g, srcs, streams, luma, n_intra, prev_model, seen)
        if want is None:
            with pytest.raises(ValueError):
                pkg.submit_plan(q, c_src, c_st, luma, n_intra, prev_lib)
            counts["refused"] += 1
            return
        got = pkg.submit_plan(q, c_src, c_st, luma, n_intra, prev_lib)
        what = "case %r call %d" % (case, call)
        # ---- equality with the restatement
        for (k, t), p in want["pics"].items():
            assert {f: got["pics"][k * F + t][f] for f in PIC_FIELDS} == {f: p[f] for f in PIC_FIELDS}, (what, k, t)
        assert got["pairs"] == want["pairs"], what
        assert got["ext"] == want["ext"] and got["remedy_streams"] == want["remedy_streams"], what

        def flat(j):
            return dict(pic=j["pic"][0] * F + j["pic"][1], ref_recon_slot=j["ref"], recon_slot=j["recon"], out_slot=j["out"],
                        border_hint=j["hint"], remedy=j["remedy"])
        assert got["remedy"] == [flat(j) for j in want["remedy"]], what
        assert got["jobs"] == [flat(j) for j in want["jobs"]], what
        assert got["calls"] == want["calls"] and got["dropped"] == want["dropped"], what
        for s in range(S):
            assert {f: getattr(c_src[s], f) for f in SRC_FIELDS} == srcs[s], what
        for k in range(N):
            lib_st = (c_st[k].has_recon, c_st[k].border_skipped, c_st[k].recon_dropped, c_st[k].next_gop)
            assert lib_st == (streams[k]["has_recon"], streams[k]["border_skipped"], streams[k]["recon_dropped"], int(want["next_gop"][k])), what
            if not chains:
                assert k + N * c_st[k].rpar == streams[k]["cur"], what
        assert list(q.carry) == g["carry"], what
        # ---- invariants, on the library's tables
        P = got["pics"]
        first_p = [P[k * F]["isP"] for k in range(N)]
        for k in range(N):                                   # 6. a dropped last picture the call predicts from is remedied exactly once
            n = got["remedy_streams"].count(k)               # (decided before the motion search: a candidate turned intra after it was remedied too)
            assert n <= 1 and (n == 0 or before[k]["recon_dropped"]) and (n == 1 or not (before[k]["recon_dropped"] and first_p[k])), what
        for j in got["remedy"]:
            k = j["pic"] // F
            if j["ref_recon_slot"] >= 0:
                assert writer[j["ref_recon_slot"]] == (k, coded[k] - 2), what
            assert j["recon_slot"] >= 0 and j["recon_slot"] != j["ref_recon_slot"] and j["border_hint"] == 0, what
            writer[j["recon_slot"]] = (k, coded[k] - 1)
        assert len(set(j["out_slot"] for j in got["remedy"])) == len(got["remedy"]), what
        half = range(par * N * F, (par + 1) * N * F)
        assert len(set(j["out_slot"] for j in got["jobs"])) == len(got["jobs"]) == nf * N, what        # 8.
        assert all(j["out_slot"] in half for j in got["jobs"] + got["remedy"]), what
        call_of = {}
        for ci, c in enumerate(got["calls"]):
            for step in range(c["nsteps"]):
                js = got["jobs"][c["first"] + step * c["njobs"]:c["first"] + (step + 1) * c["njobs"]]
                if chains:                                   # 3. chains coded side by side never share a pair
                    prs = [max(j["recon_slot"], j["ref_recon_slot"]) // 2 for j in js if max(j["recon_slot"], j["ref_recon_slot"]) >= 0]
                    assert len(set(prs)) == len(prs), what
                    assert all(pr <= chains for pr in prs), what
                for j in js:
                    call_of[j["pic"]] = ci
        assert len(call_of) == nf * N, what                  # every picture is in exactly one call
        len0 = next((t for t in range(1, nf) if not P[t]["isP"]), nf) if chains else 0
        last0 = max((i for i, j in enumerate(got["jobs"]) if j["pic"] < len0), default=-1)
        for i, j in enumerate(got["jobs"]):
            k, t = divmod(j["pic"], F)
            p = P[j["pic"]]
            n = coded[k] + t
            if j["ref_recon_slot"] >= 0:                     # 1. the reference is the stream's picture before, still in its slot
                assert p["isP"] and writer.get(j["ref_recon_slot"]) == (k, n - 1), (what, j)
            else:
                assert not p["isP"], what
            assert j["recon_slot"] < 0 or j["recon_slot"] != j["ref_recon_slot"], what       # 2.
            if j["recon_slot"] >= 0:
                assert p["is_ref"], what
                writer[j["recon_slot"]] = (k, n)
            elif p["is_ref"]:                                # 5. dropped: only where nobody reads it
                if t + 1 < nf:
                    assert not P[j["pic"] + 1]["isP"] and not serial and not keep_all, what
                else:
                    assert c_st[k].next_gop and not abr and not keep_all and not chains, what
            if chains and first_p[0] and i <= last0 and t >= len0:       # 4. the carried pair is left alone while its chain goes on
                assert carry[0] not in (j["recon_slot"] // 2, j["ref_recon_slot"] // 2), what
            if j["border_hint"]:                             # 7. only where the next picture is in this call or starts a GOP
                if t + 1 < nf and P[j["pic"] + 1]["isP"]:
                    assert call_of[j["pic"] + 1] == call_of[j["pic"]], what
                elif t + 1 == nf:
                    assert c_st[k].next_gop, what
        for k in range(N):
            coded[k] += nf
        counts["calls"] += 1
        counts["jobs"] += len(got["jobs"])
        prev_model, prev_lib = want["pics"], got["_pics"]
        carry, gcount, par, nf_prev = list(q.carry), gcount + nf, par ^ 1, nf
        # ---- what a caller does between calls: dsv1_batch_set_fnum (forwards, backwards, onto a GOP start), forced metadata
        for s in range(S):
            r = rnd.random()
            nxt = srcs[s]["next_fnum"]
            if r < 0.15:
                nxt = (nxt + rnd.randint(1, 20)) & SP.M32
            elif r < 0.40:
                nxt = max(0, nxt - rnd.randint(1, max(1, gop))) if nxt < 0x80000000 else nxt
            elif r < 0.50 and gop:
                nxt = (srcs[s]["prev_gop"] + gop) & SP.M32
            srcs[s]["next_fnum"] = c_src[s].next_fnum = nxt
            if rnd.random() < 0.1:
                srcs[s]["force_metadata"] = c_src[s].force_metadata = 1


def test_submit_plan_equals_the_restatement_and_keeps_its_invariants(pkg):
    seen, counts = collections.Counter(), collections.Counter()
    for case in sequences():
        run_sequence(pkg, case, seen, counts)
    print("submit plan: %d calls, %d jobs, %d refused; classes: %s" % (counts["calls"], counts["jobs"], counts["refused"],
                                                                       ", ".join("%s %d" % (c, seen[c]) for c in SP.CLASSES)))
    empty = [c for c in SP.CLASSES if not seen[c]]
    assert not empty, "classes the cases never reach: %s" % empty


def test_cases_cover_the_lists(pkg):
    cs = sequences()
    assert {c[1] for c in cs} == {1, 2, 3} and {c[2] for c in cs} == {1, 3} and {c[3] for c in cs} == {1, 3, 4, 6, 12}
    assert {c[4] for c in cs} == {0, 1, 4, 6, 12} and {c[5] for c in cs} == set(MODES) and {c[6] for c in cs} == {0, 1, 2, 4}
    assert {c[7] for c in cs} == {False, True} and {c[9] for c in cs} == {1, 2, 3, 4}


def test_submit_plan_refuses(pkg):
    def q(**kw):
        d = dict(S=1, R=1, F=4, nf=4, chains=0, gcount=0, par=0, npix_small=NPIX, nblk=NBLK, intra_pct_thresh=THRESH, abr=0, serial=0,
                 keep_all=0, nf_prev=0)
        d.update(kw)
        return pkg.SubmitQuery(*[d[k] for k in ("S", "R", "F", "nf", "chains", "gcount", "par", "npix_small", "nblk", "intra_pct_thresh",
                                               "abr", "serial", "keep_all", "nf_prev")], (pkg._C.c_int * 2)(-1, -1))

    def go(qq):
        N = qq.S * qq.R
        src = [pkg.SubmitSrc(0, 0xFFFFFFFF, 4, 1, 0, 0, 4) for _ in range(max(qq.S, 1))]
        return pkg.submit_plan(qq, src, [pkg.SubmitStream() for _ in range(max(N, 1))], [0] * ((2 * qq.F + 1) * max(qq.S, 1)), [0] * (max(N, 1) * qq.F))
    assert len(go(q())["jobs"]) == 4
    for bad in (q(nf=5), q(S=2, nf=3), q(abr=1, chains=2), q(serial=1), q(S=2, chains=1), q(npix_small=0)):
        with pytest.raises(ValueError):
            go(bad)
    # chain mode, a stream renumbered so that its first picture ever is a P picture: no reference picture on the device
    with pytest.raises(ValueError):
        src = [pkg.SubmitSrc(3, 0, 4, 0, 0, 0, 4)]
        pkg.submit_plan(q(chains=2), src, [pkg.SubmitStream()], [0] * 9, [0] * 4)
