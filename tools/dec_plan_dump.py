"""Writes the cases tools/dec_plan_host.cpp walks under a sanitizer: the decoder calls of tests/dec_cases.py under a few switch settings,
its header planes and the refused calls of tests/test_dec_plan_host.py, each with the answer of the device-free query dsvg_decode_plan.
    python tools/dec_plan_dump.py cases.bin
Per case, little-endian int32 unless said: DecGeo (n_recon, max_jobs, nblk, cw[3], ch[3], nchunks[3], sym_ok[2], ov[2], mc_patch, nbh, nbv,
blk_w, blk_h, hs, vs, pw[3], ph[3], second_stream); no_dec_sym, no_dec_sym_I, one_stream, no_mc_patch, no_inplace_pred, force32, profiled,
draw_mode, njobs as passed, jobs in the file, the query's return code; per job ref, recon, quant, has vectors, has flags, plane_len[3],
bytes behind each plane pointer[3] (-1: a null pointer), then its vector table (nblk dsvg_mv), flag table (nblk bytes) and payloads.  Then
the answer: 256 bytes of error text for a refused call, else int64: nI, blob, nmeta, max_entries, max_chunks, insym, f0, anysym,
scatter_one, resolve, fork, mc, ex0, ey0, iln, draw0, draw1, order / path / wide / inplace [njobs], dec_sym / dc / runs / len / bitpos /
blob_off / meta_off [3 njobs], ilist[iln]."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import dec_cases as K                     # noqa: E402


def i32(*v):
    return np.array(v, dtype="<i4").tobytes()


def write_case(f, c, switches=0, force32=0, draw_mode=0, njobs=None):
    P = K.pkg()
    njobs = c.njobs if njobs is None else njobs
    try:
        plan, rc, text = c.plan(switches, force32, draw_mode, njobs), 0, ""
    except P.DecodeRefused as e:
        plan, rc, text = None, e.rc, e.text
    g = K.Call(c.geom, "P", max_jobs=max(c.max_jobs, 1)).plan(switches & (P.DEC_NO_SYM_OV | P.DEC_NO_MC_FUSION))     # the geometry record
    cd, pd = [c.coef_dims(p) for p in range(3)], [c.plane_dims(p) for p in range(3)]
    f.write(i32(c.n_recon, c.max_jobs, c.nblk, *[d[0] for d in cd], *[d[1] for d in cd], *g["nchunks"], *g["sym_ok"], *g["ov"], g["mc_patch"],
                c.nbh, c.nbv, c.bw, c.bh, c.hs, c.vs, *[d[0] for d in pd], *[d[1] for d in pd], int(c.max_jobs >= 16)))
    f.write(i32(*[int(bool(switches & b)) for b in (P.DEC_NO_SYM, P.DEC_NO_SYM_I, P.DEC_ONE_STREAM, P.DEC_NO_MC_PATCH, P.DEC_NO_INPLACE_PRED)],
                int(force32), int(bool(switches & P.DEC_PROFILED)), draw_mode, njobs, len(c.jobs), rc))
    for j in c.jobs:
        f.write(i32(j["ref"], j["recon"], j["quant"], int(j["mv"] is not None), int(j["st"] is not None), *j["lens"],
                    *[-1 if a is None else min(len(a), ln) for a, ln in zip(j["planes"], j["lens"])]))
        if j["mv"] is not None:
            f.write(j["mv"].tobytes())
        if j["st"] is not None:
            f.write(j["st"].tobytes())
        for a, ln in zip(j["planes"], j["lens"]):
            if a is not None:
                f.write(a.tobytes()[:min(len(a), ln)])
    if plan is None:
        f.write(text.encode().ljust(256, b"\0"))
        return
    p = plan
    f.write(np.array([p[k] for k in ("nI", "blob", "nmeta", "max_entries", "max_chunks", "insym", "f0", "anysym", "scatter_one", "resolve", "fork",
                                     "mc", "ex0", "ey0", "iln", "draw0", "draw1")], dtype="<i8").tobytes())
    for k in ("order", "path", "wide", "inplace", "dec_sym", "dc", "runs", "len", "bitpos", "blob_off", "meta_off", "ilist"):
        f.write(p[k].astype("<i8").tobytes())


def refused_calls():
    """the refusals of tests/test_dec_plan_host.py, one or two changes each: (call, njobs as passed or None)"""
    def call():
        return K.Call("96x64", "PIPP", seed=3, max_jobs=4)

    def changed(fn, njobs=None):
        c = call()
        fn(c)
        return c, njobs

    def job(i, **kw):
        return lambda c: c.jobs[i].update(kw)

    def plane(i, q, data=False, length=None):
        def fn(c):
            if data is None:
                c.jobs[i]["planes"][q] = None
            if length is not None:
                c.jobs[i]["lens"][q] = length
        return fn
    yield changed(lambda c: None, 0)
    yield changed(lambda c: None, -1)
    yield changed(lambda c: setattr(c, "max_jobs", 3))
    for i, q in ((2, 0), (1, 2), (3, 1)):
        yield changed(plane(i, q, data=None))
        yield changed(plane(i, q, length=10 ** 9))
    for kw in (dict(recon=-1), dict(recon=12), dict(st=None)):
        for i in (1, 2, 3):
            yield changed(job(i, **kw))
    yield changed(job(2, ref=12))
    yield changed(job(2, mv=None))
    yield changed(lambda c: (job(1, recon=-1)(c), plane(3, 2, length=10 ** 9)(c)))
    yield changed(lambda c: (job(0, st=None)(c), job(1, st=None)(c)))


def main(path):
    P = K.pkg()
    n = 0
    with open(path, "wb") as f:
        for name, c in K.calls():
            for sw, f32, draw in ((0, 0, 0), (P.DEC_NO_SYM_I | P.DEC_PROFILED, 0, 3), (P.DEC_NO_SYM_OV | P.DEC_NO_MC_PATCH | P.DEC_ONE_STREAM, 0, 0),
                                  (P.DEC_NO_INPLACE_PRED | P.DEC_NO_MC_FUSION, 1, 1), (P.DEC_NO_SYM, 0, 0)):
                write_case(f, c, sw, f32, draw)
                n += 1
        for hname, data, length in K.header_planes():
            c = K.Call("250x130", "PIP", seed=5)
            for t, q in ((0, 0), (1, 2), (2, 1)):
                c.set_plane(t, q, data, length)
            write_case(f, c)
            n += 1
        for c, njobs in refused_calls():
            write_case(f, c, njobs=njobs)
            n += 1
    print("%d cases" % n)


if __name__ == "__main__":
    main(sys.argv[1])
