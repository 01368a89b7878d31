"""Writes the cases tools/batch_plan_host.cpp walks under a sanitizer: the coding calls of tests/batch_cases.py (those of up to 200 000
blocks, under a few switch settings) and the refused calls of tests/test_batch_plan_host.py, each with the answer of the device-free
query dsvg_code_batch_plan.
    python tools/batch_plan_dump.py cases.bin
Per case, little-endian int32 unless said: BatchGeo (nblk, n_recon, n_src, max_jobs, out_slots, rc_slots, mc_fused, code_streams,
lazy_border, blk_w, blk_h, nbh, hs, vs, w[2], h[2]); no_small_split, no_par_enqueue, profiled, nsteps, njobs, has_rc, vector tables,
flag tables, jobs in the file, the query's return code; the vector tables (nblk dsvg_mv each) and flag tables (nblk bytes each); per job
src, ref, recon, quant, vector table or -1, flag table or -1, out, no_intra_blocks, has_reach, mv_reach[4], border_hint; per job rc_slot,
prefix_len, forced_intra if has_rc.  Then the answer: 256 bytes of error text for a refused call, else base, total, ng, gk[5], iln,
nmv, nst, mv_contig, par_enqueue, nI[nsteps], order / mvu / stu / mvcp / stcp / rc_next [total], ext[total * 8], ioff / icnt / noint /
keeps [nsteps * ng], ilist[iln]."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import batch_cases as K                     # noqa: E402


def i32(*v):
    return np.array(v, dtype="<i4").tobytes()


def write_case(f, sc, switches=0, code_streams=None):
    P = K.pkg()
    cs = sc.code_streams if code_streams is None else code_streams
    try:
        plan, rc, text = sc.plan(switches, cs), 0, ""
    except P.BatchRefused as e:
        plan, rc, text = None, e.rc, e.text
    fusable = P.dispatch_plan(sc.w, sc.h, sc.fmt)["fusable"]
    f.write(i32(sc.nblk, sc.n_recon, sc.n_src, sc.max_jobs, max(sc.out_slots, sc.max_jobs), max(sc.n_recon, sc.max_jobs),
                int(fusable and not switches & P.BATCH_NO_MC_FUSION), cs, int(not switches & P.BATCH_NO_LAZY_BORDER), sc.bw, sc.bh, sc.nbh, sc.hs, sc.vs,
                sc.w, -(-sc.w >> sc.hs), sc.h, -(-sc.h >> sc.vs)))
    f.write(i32(int(bool(switches & P.BATCH_NO_SMALL_SPLIT)), int(bool(switches & P.BATCH_NO_PAR_ENQUEUE)), int(bool(switches & P.BATCH_PROFILED)),
                sc.nsteps, sc.njobs, int(sc.rc is not None), len(sc.mv_tables), len(sc.st_tables), len(sc.jobs), rc))
    for t in sc.mv_tables:
        f.write(t.tobytes())
    for t in sc.st_tables:
        f.write(t.tobytes())
    for j in sc.jobs:
        f.write(i32(j["src"], j["ref"], j["recon"], j["quant"], -1 if j["mv"] is None else j["mv"], -1 if j["st"] is None else j["st"], j["out"],
                    j["no_intra"], j["has_reach"], *j["reach"], j["hint"]))
    if sc.rc is not None:
        for r in sc.rc:
            f.write(i32(*r))
    if plan is None:
        f.write(text.encode().ljust(256, b"\0"))
        return
    p = plan
    f.write(i32(p["base"], p["total"], p["ng"], *(list(p["gk"]) + [0] * (5 - len(p["gk"]))), p["iln"], p["nmv"], p["nst"], p["mv_contig"], p["par_enqueue"]))
    for k in ("nI", "order", "mvu", "stu", "mvcp", "stcp", "rc_next", "ext", "ioff", "icnt", "noint", "keeps", "ilist"):
        f.write(p[k].astype("<i4").tobytes())


def refused_calls():
    """the refusals of tests/test_batch_plan_host.py::test_refusals, one change each"""
    def call(rc=False):
        return K.build("96x64", "c", 4, 3, rc=rc)
    def changed(fn, rc=False):
        sc = call(rc)
        fn(sc)
        return sc
    def attr(**kw):
        return lambda sc: [setattr(sc, k, v) for k, v in kw.items()]
    def job(i, **kw):
        return lambda sc: sc.jobs[i].update(kw)
    def rcj(i, v):
        return lambda sc: sc.rc.__setitem__(i, v)
    yield changed(attr(max_jobs=3))
    yield changed(attr(out_slots=11))
    yield changed(attr(nsteps=0))
    yield changed(attr(njobs=0))
    yield changed(attr(nsteps=-1))
    yield changed(lambda sc: [j.update(out=j["out"] + 4) for j in sc.jobs])
    yield changed(job(5, out=-1))
    yield changed(job(6, out=14))
    yield changed(job(5, src=-1))
    yield changed(job(5, src=12))
    yield changed(job(5, recon=8))
    yield changed(job(5, ref=8))
    yield changed(job(5, st=None))
    yield changed(lambda sc: next(j for j in sc.jobs[4:] if j["ref"] >= 0).update(mv=None))
    yield changed(rcj(5, (8, 0, 0)), True)
    yield changed(rcj(2, (2, -1, 0)), True)
    yield changed(rcj(6, (7, 0, 0)), True)
    yield changed(rcj(3, (1, 0, 0)), True)


def main(path):
    P = K.pkg()
    n = 0
    with open(path, "wb") as f:
        for sc in K.scenarios():
            if sc.total * sc.nblk > 200000:
                continue
            write_case(f, sc)
            n += 1
            if sc.nsteps >= 8 or sc.S in (16, 17):
                for sw in (P.BATCH_NO_SMALL_SPLIT, P.BATCH_NO_LAZY_BORDER | P.BATCH_PROFILED, P.BATCH_NO_MC_FUSION | P.BATCH_NO_PAR_ENQUEUE):
                    write_case(f, sc, sw)
                    n += 1
                write_case(f, sc, 0, 1)
                n += 1
        for sc in refused_calls():
            write_case(f, sc)
            n += 1
    print("%d cases" % n)


if __name__ == "__main__":
    main(sys.argv[1])
