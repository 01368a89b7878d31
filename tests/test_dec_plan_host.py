"""The plan of a decoder call (csrc/dsvg_dec_plan.h: plan_decode, every check and every host decision of dsvg_decode_pictures), asked
through the device-free query dsvg_decode_plan, on the CPU.

Every decision is held against a definition written out HERE from the call as the caller states it (tests/dec_cases.py) -- never against
another field of the plan: device order, the payload blob and the parse records, the plane header (against the bit reader of
tests/hzdec_plan.py, bounded as the decoder's is), the grids, which pictures and planes go to the int16 symbol planes, one scatter launch
or three (also against hzdec_plan.scatter_launches), the resolve launch, the fork, the motion compensation path with (ex0, ey0) and the
intra list (a per-block numpy restatement), in-place prediction, the overlay's range, the limits, and every refusal with its code, its
text and the first-failure order."""
import itertools

import numpy as np
import pytest

import _cabi as A
import dec_cases as K
import hz_plan as H
import hzdec_plan as D

P = K.pkg()
ERR_ARG = -2
SW = dict(no_sym=P.DEC_NO_SYM, no_sym_i=P.DEC_NO_SYM_I, one_stream=P.DEC_ONE_STREAM, no_mc_patch=P.DEC_NO_MC_PATCH,
          no_inplace=P.DEC_NO_INPLACE_PRED, no_sym_ov=P.DEC_NO_SYM_OV, no_mc_fusion=P.DEC_NO_MC_FUSION, profiled=P.DEC_PROFILED)
# patch motion compensation (mc_fusable): the issue's two, the rest from the geometry query the forward plan's tests hold
FUSABLE = {"96x64": True, "384x240": False}
CALLS = list(K.calls())
SMALL = [(n, c) for n, c in CALLS if c.geom != "1080p"]


def fusable(c):
    return FUSABLE.get(c.geom, bool(P.dispatch_plan(c.w, c.h, c.fmt)["fusable"]))


def device_order(c):
    return [i for i, k in enumerate(c.kinds) if k == "I"] + [i for i, k in enumerate(c.kinds) if k == "P"]


def plane_ov(c, g):
    return H.overlaps(*c.coef_dims(g))


def sym_ok(c, g, sw):
    """the plane kind's coefficients start 4-aligned in a job's coefficient block, and DSV1_NO_DEC_SYM_OV keeps planes with shared cells out"""
    off = [0, c.coef_dims(0)[0] * c.coef_dims(0)[1]]
    off.append(off[1] + c.coef_dims(1)[0] * c.coef_dims(1)[1])
    return off[1 if g else 0] % 4 == 0 and off[2] % 4 == 0 and not (plane_ov(c, g) and sw & SW["no_sym_ov"])


class BoundedBits(D.Bits):
    """the decoder's reader: `length` bytes, past them every bit reads as 1 and the position stays"""

    def __init__(self, data, length):
        super().__init__(bytes(data[:length]) + b"\0")
        self.end = 8 * length

    def bit(self):
        return 1 if self.pos >= self.end else super().bit()


def header(data, length):
    dc, runs, pos = D.read_header(BoundedBits(data, length))
    return dc, runs, pos


def expected(c, sw=0, force32=False, draw_mode=0):
    """every decision of the call, from the caller's statement of it"""
    e = {}
    order = device_order(c)
    nI, n = c.kinds.count("I"), c.njobs
    e["order"], e["nI"] = order, nI
    off = moff = 0
    e["blob_off"], e["meta_off"] = [], []
    max_entries = max_chunks = 0
    e["hdr"] = []
    for i in order:
        j = c.jobs[i]
        bo, mo, hd = [], [], []
        for p in range(3):
            ln = j["lens"][p]
            bo.append(off)
            mo.append(moff)
            off += (ln + 64 + 15) & ~15                    # 64 guard bytes behind every plane, planes 16-aligned
            moff += ln // 16 + 2                           # a record per 128-bit chunk, two spare
            dc, runs, pos = header(j["planes"][p].tobytes(), ln)
            hd.append((dc, runs, pos, ln))
            nchunks = H.geometry(*c.coef_dims(p))[2]
            max_entries = max(max_entries, min(runs, nchunks * D.HZ_CHUNK - 1) + 1)
            max_chunks = max(max_chunks, ln // 16 + 2)
        e["blob_off"].append(bo)
        e["meta_off"].append(mo)
        e["hdr"].append(hd)
    e["blob"], e["nmeta"], e["max_entries"], e["max_chunks"] = off, moff, max_entries, max_chunks
    ok = [sym_ok(c, g, sw) for g in (0, 1)]
    sparse = not (sw & SW["no_sym"]) and not force32
    sparse_i = sparse and ok[0] and ok[1] and not (sw & SW["no_sym_i"])
    e["path"], e["dec_sym"], e["wide"], e["inplace"] = [], [], [], []
    for i in order:
        j = c.jobs[i]
        isP = c.kinds[i] == "P"
        path = (2 if sparse else 0) if isP else (1 if sparse_i else 0)
        e["path"].append(path)
        e["dec_sym"].append([1, 1, 1] if path == 1 else [int(ok[0]), int(ok[1]), int(ok[1])] if path == 2 else [0, 0, 0])
        e["wide"].append(int(path == 1))
        e["inplace"].append(int(path == 2 and j["recon"] != j["ref"] and not (sw & SW["no_inplace"])))
    sym_I = sparse_i and nI > 0
    e["insym"] = 0 if not sparse else (1 if sym_I else 0) | (2 if ok[0] else 0) | (4 if ok[1] else 0)
    e["f0"] = 0 if sym_I else nI
    # some plane of some picture of the call is on the symbol path
    e["anysym"] = int(any(any(d) for d in e["dec_sym"]))
    # one scatter launch where EVERY plane of every picture is
    e["scatter_one"] = int(all(all(d) for d in e["dec_sym"]))
    # the resolve kernel where a plane with shared cells is on the symbol path; the P pictures' planes decide (sym_ok is theirs)
    e["resolve"] = int(bool(e["anysym"]) and any(plane_ov(c, g) and ok[g] for g in (0, 1)))
    second = c.max_jobs >= 16
    e["fork"] = int(n > nI and n >= 4 and not (sw & SW["one_stream"]) and not (sw & SW["profiled"]) and second)
    patch = fusable(c) and not (sw & SW["no_mc_fusion"])
    e["mc"] = 0 if n == nI else 2 if patch and not (sw & SW["no_mc_patch"]) else 1
    e["draw"] = (nI, n) if draw_mode and n > nI else (n, n)
    return e


def ragged_from(c):
    """(ex0, ey0): the first block column / row that holds a ragged 8x8 patch in SOME plane, the grid's size where none does"""
    ex0, ey0 = c.nbh, c.nbv
    for p in range(3):
        pw, ph = c.plane_dims(p)
        bw, bh = (c.bw >> c.hs, c.bh >> c.vs) if p else (c.bw, c.bh)
        if pw % 8:
            ex0 = min(ex0, (pw // 8 * 8) // bw)
        if ph % 8:
            ey0 = min(ey0, (ph // 8 * 8) // bh)
    return ex0, ey0


def intra_list(c, ex0, ey0):
    """per P picture in device order, per block: intra, or in a block column / row from (ex0, ey0) on"""
    out, k = [], 0
    for i in device_order(c):
        if c.kinds[i] != "P":
            continue
        b = np.arange(c.nblk)
        take = (c.jobs[i]["mv"]["mode"] != 0) | (b % c.nbh >= ex0) | (b // c.nbh >= ey0)
        out.append(k * c.nblk + b[take])
        k += 1
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


PARTS = ("layout", "header", "paths", "launch", "mc")       # a test checks one part: a wrong decision fails the tests named for it alone


def check(c, sw=0, force32=False, draw_mode=0, what=PARTS):
    p = c.plan(sw, force32, draw_mode)
    e = expected(c, sw, force32, draw_mode)
    tag = "%s %s sw %#x force32 %d draw %d" % (c.geom, c.kinds, sw, force32, draw_mode)
    if "layout" in what:
        assert list(p["order"]) == e["order"] and p["nI"] == e["nI"], tag
        assert p["blob_off"].tolist() == e["blob_off"] and p["blob"] == e["blob"], tag
        assert p["meta_off"].tolist() == e["meta_off"] and p["nmeta"] == e["nmeta"], tag
        assert p["max_chunks"] == e["max_chunks"], tag
    if "header" in what:
        got = [[(int(p["dc"][t, q]), int(p["runs"][t, q]), int(p["bitpos"][t, q]), int(p["len"][t, q])) for q in range(3)] for t in range(c.njobs)]
        assert got == e["hdr"], tag
        assert p["max_entries"] == e["max_entries"], tag
    if "paths" in what:
        for k in ("path", "dec_sym", "wide", "inplace"):
            assert p[k].tolist() == e[k], (tag, k)
        for k in ("insym", "f0", "anysym"):
            assert p[k] == e[k], (tag, k)
    if "launch" in what:
        for k in ("scatter_one", "resolve", "fork"):
            assert p[k] == e[k], (tag, k)
        assert (p["draw0"], p["draw1"]) == e["draw"], tag
        if all(sym_ok(c, g, sw) for g in (0, 1)):             # (hzdec_plan's restatement is for geometries whose planes all qualify)
            one = D.scatter_launches(c.kinds, sym=not (sw & SW["no_sym"]) and not force32, sym_i=not (sw & SW["no_sym_i"])) == 1
            assert bool(p["scatter_one"]) == one, tag
    if "mc" in what:
        assert p["mc"] == e["mc"], tag
        if e["mc"] == 2:
            assert (p["ex0"], p["ey0"]) == ragged_from(c), tag
            assert p["ilist"].tolist() == intra_list(c, *ragged_from(c)).tolist(), tag
        else:
            assert p["iln"] == 0, tag
    return p


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in CALLS])
@pytest.mark.parametrize("part", PARTS)
def test_call(part, name):
    """every geometry x kinds x size, no switch"""
    check(dict(CALLS)[name], what=(part,))


@pytest.mark.parametrize("switch", list(SW))
@pytest.mark.parametrize("part", PARTS)
def test_each_switch_alone(part, switch):
    for name, c in SMALL:
        check(c, SW[switch], what=(part,))


@pytest.mark.parametrize("part", PARTS)
def test_force32_profiled_and_draw_modes(part):
    for name, c in SMALL:
        check(c, force32=True, what=(part,))
        check(c, SW["profiled"], draw_mode=3, what=(part,))
        check(c, draw_mode=1, what=(part,))
        check(c, SW["no_sym_i"], force32=True, draw_mode=7, what=(part,))


@pytest.mark.parametrize("part", PARTS)
def test_switch_pairs_on_a_mixed_call(part):
    c = dict(CALLS)["250x130-mixed-4-mj16"]
    for a, b in itertools.combinations(SW.values(), 2):
        check(c, a | b, what=(part,))


def test_geometry_record():
    """what the plan read of the context: blocks, shared cells, symbol planes, scan chunks, the second stream, the patch kernel"""
    for name, c in CALLS:
        for sw in (0, SW["no_sym_ov"], SW["no_mc_fusion"]):
            p = c.plan(sw)
            assert (p["nblk"], p["nbh"]) == (c.nblk, c.nbh), name
            assert p["ov"] == tuple(int(plane_ov(c, g)) for g in (0, 1)), name
            assert p["sym_ok"] == tuple(int(sym_ok(c, g, sw)) for g in (0, 1)), name
            assert p["nchunks"] == tuple(H.geometry(*c.coef_dims(q))[2] for q in range(3)), name
            assert p["second_stream"] == int(c.max_jobs >= 16), name
            assert p["mc_patch"] == int(fusable(c) and not sw & SW["no_mc_fusion"]), name
    ov = {g: tuple(plane_ov(K.Call(g, "P"), k) for k in (0, 1)) for g in K.GEOMS}
    assert ov["250x130"] == (True, True) and ov["40x32"] == (False, True) and ov["96x64"] == (False, False), ov


def test_the_fork_threshold():
    """the second stream takes the motion compensation from four pictures on, where there is a P picture and a second stream"""
    want = {("PPP", 16): 0, ("PPPP", 16): 1, ("PPPP", 4): 0, ("IIII", 16): 0, ("IIIP", 16): 1, ("P", 16): 0}
    for (kinds, mj), fork in want.items():
        c = K.Call("96x64", kinds, max_jobs=mj)
        assert c.plan()["fork"] == fork, (kinds, mj)
        assert c.plan(SW["one_stream"])["fork"] == 0 and c.plan(SW["profiled"])["fork"] == 0


def test_limits():
    """a P picture of 8-bit video: detail <= 4 x the LL below, LL = 4/5 of that, a dequantised value <= twice its coefficient; wide: 2^30 - 1"""
    lim = [0] * 16
    ll = 512
    lim[1] = 2 * 510
    for lv in range(2, 16):
        det = 4 * ll
        lim[lv] = min(2 * det, 0x3fffffff)
        ll = min(det * 4 // 5, 0x1fffffff)
    lim[0] = min(2 * ll, 0x3fffffff)
    p = K.Call("96x64", "IP").plan()
    assert p["lim"][0].tolist() == lim and p["lim"][1].tolist() == [0x3fffffff] * 16
    assert p["wide"].tolist() == [1, 0]


@pytest.mark.parametrize("geom", ["96x64", "250x130", "1080p"])
@pytest.mark.parametrize("hp", K.header_planes(), ids=[h[0] for h in K.header_planes()])
def test_plane_header(geom, hp):
    """the header read against hzdec_plan's reader, bounded: a plane of 0, 1, 4, 5 and 6 bytes reads ones past its end; a DC whose code
    crosses a byte boundary; a count above the clamp of max_entries and a negative one"""
    name, data, length = hp
    c = K.Call(geom, "PIP", seed=5)
    for t, q in ((0, 0), (1, 2), (2, 1)):
        c.set_plane(t, q, data, length)
    p = check(c, what=("header",))
    dc, runs, pos = header(data, length)
    t = list(p["order"]).index(1)
    assert (p["dc"][t, 2], p["runs"][t, 2], p["bitpos"][t, 2], p["len"][t, 2]) == (dc, runs, pos, length)
    assert pos <= 8 * length
    if name == "whole":
        assert dc == -400000 and runs == 77 and pos == 72
    if name == "cut-0":
        assert (dc, runs, pos) == (0, -1, 0)
    if name == "count-clamped":
        cap = max(H.geometry(*c.coef_dims(q))[2] for q in range(3)) * D.HZ_CHUNK
        assert runs == 10 ** 8 and p["max_entries"] <= cap
        if geom == "96x64":
            assert p["max_entries"] == H.geometry(96, 64)[2] * D.HZ_CHUNK
    if name == "count-neg":
        assert runs < 0


@pytest.mark.parametrize("geom", ["96x64", "250x130", "384x240", "1080p"])
def test_intra_list_and_ragged_patches(geom):
    """the intra list and (ex0, ey0) per block, on geometries with ragged 8x8 patches (250x130: luma 250 = 31 patches + 2, chroma 65 =
    8 patches + 1) and without; every block intra, none intra"""
    for kinds, fill in (("PIPP", None), ("PP", 0), ("PP", 1)):
        c = K.Call(geom, kinds, seed=11)
        for j in c.jobs:
            if fill is not None and j["mv"] is not None:
                j["mv"]["mode"] = fill
        p = check(c, what=("mc",))
        if fusable(c):
            assert p["mc"] == 2
            if geom == "96x64":
                assert (p["ex0"], p["ey0"]) == (c.nbh, c.nbv)
                if fill == 0:
                    assert p["iln"] == 0
            if geom == "250x130":
                # luma 250 / 130 and chroma 125 / 65 all end in a ragged patch: the last block column and row at least
                assert p["ex0"] < c.nbh and p["ey0"] < c.nbv
            if fill == 1:
                assert p["iln"] == c.kinds.count("P") * c.nblk
        else:
            assert p["mc"] == 1 and p["iln"] == 0


def test_a_geometry_below_the_contexts_minimum_is_refused():
    """20x30 is a plane size of the entropy stage's tests, not a context's: dsvg_ctx_create takes 32x32 and more, and the query answers as it does"""
    c = K.Call("96x64", "P")
    with pytest.raises(P.DecodeRefused) as e:
        P.decode_plan(20, 30, A.SUBSAMP_420, c.n_recon, c.max_jobs, 0, False, 0, 1, c.c_jobs())
    assert e.value.rc == ERR_ARG and e.value.text == "bad ctx_create arguments"


# ---------------------------------------------------------------------------------------------------------------------------
def refused(c, njobs=None):
    with pytest.raises(P.DecodeRefused) as e:
        c.plan(njobs=njobs)
    return e.value.rc, e.value.text


def base_call():
    return K.Call("96x64", "PIPP", seed=3, max_jobs=4)        # device order 1, 0, 2, 3


def test_refusals():
    """each check, tripped by a job that is not the first in the caller's order: the code, the text with the CALLER's index"""
    c = base_call()
    c.plan()
    assert refused(c, njobs=0) == (ERR_ARG, "bad decode_pictures arguments")
    assert refused(c, njobs=-1) == (ERR_ARG, "bad decode_pictures arguments")
    c.max_jobs = 3
    assert refused(c) == (ERR_ARG, "bad decode_pictures arguments")
    bound = [c.coef_dims(q)[0] * c.coef_dims(q)[1] * 8 for q in range(3)]
    for i, q in ((2, 0), (1, 2), (3, 1)):
        c = base_call()
        c.jobs[i]["planes"][q] = None
        assert refused(c) == (ERR_ARG, "plane %d of decode job %d: bad length" % (q, i))
        c = base_call()
        c.jobs[i]["lens"][q] = bound[q] + 1               # (refused before a byte of it is read)
        assert refused(c) == (ERR_ARG, "plane %d of decode job %d: bad length" % (q, i))
        c = base_call()
        c.set_plane(i, q, bytes(bound[q]))                 # the bound itself passes
        c.plan()
    for change in (dict(recon=-1), dict(recon=12), dict(ref=12), dict(st=None)):
        for i in (1, 2, 3):
            c = base_call()
            c.jobs[i].update(change)
            if c.kinds[i] == "I" and "ref" in change:
                continue
            assert refused(c) == (ERR_ARG, "bad decode job %d" % i), (change, i)
    c = base_call()
    c.jobs[2]["mv"] = None
    assert refused(c) == (ERR_ARG, "bad decode job 2")
    c = base_call()
    c.jobs[1]["mv"] = None                                 # an I picture needs none
    c.plan()
    c = base_call()
    c.jobs[3]["recon"] = 11                                # the last slot passes
    c.plan()


def test_first_failure_order():
    """the call's arguments, then the planes of ALL jobs in device order, then the jobs in device order"""
    c = base_call()
    c.jobs[1]["recon"] = -1                                # device job 0 is a bad job ...
    c.jobs[3]["lens"][2] = 10 ** 9                         # ... and device job 3 has a bad plane: the plane is found first
    assert refused(c) == (ERR_ARG, "plane 2 of decode job 3: bad length")
    assert refused(c, njobs=5) == (ERR_ARG, "bad decode_pictures arguments")
    c = base_call()
    c.jobs[0]["lens"][0] = 10 ** 9                         # caller job 0 is device job 1: the I picture's plane (caller job 1) comes first
    c.jobs[1]["planes"][1] = None
    assert refused(c) == (ERR_ARG, "plane 1 of decode job 1: bad length")
    c = base_call()
    c.jobs[0]["st"] = None
    c.jobs[1]["st"] = None
    assert refused(c) == (ERR_ARG, "bad decode job 1")
    c = base_call()
    c.jobs[2]["planes"][1] = None
    c.jobs[2]["planes"][0] = None
    assert refused(c) == (ERR_ARG, "plane 0 of decode job 2: bad length")
