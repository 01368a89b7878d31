"""Every motion-compensation kernel and branch on the BUILT fields of tests/mc_cases.py, byte for byte against the oracle's operators
(oracle/orc_bmc.c, pinned to the reference by test_oracle_vs_ref.py), minus the pixels mc_cases marks unpinned.  A mismatch names the
plane, the block, its vector and mode, its path class and the first differing pixel (mc_cases.explain).

  test_operators    k_mc over the grid (dsvg_op_sub_pred / dsvg_op_add_pred) at block sizes of the test's choosing
  test_decoder      k_mc_patch plus k_mc by list, or k_mc over the grid: forked, profiled, without the prediction in place, without the
                    fused kernels, under DSV1_NO_MC_PATCH (a child process), and a picture that updates its reference in place
  test_encoder      k_fwd_mc_fast, k_fwd_mc_pix and k_mc by list, or k_mc over the grid, at quantisers 16 and 300, hints unset and set
  test_lazy_border  the border an I picture's reconstruction gets for fields of reach 0, 5 and beyond the clamp"""
import ctypes as C

import numpy as np
import pytest

import _cabi as A
import mc_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prod():
    L = A.load_prod()
    assert L.dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return L


def extreme(rng, w, h):
    """noise, and in half of the 8x8 cells columns and rows of 0 / 255 in the order 0 255 255 0: the luma taps 9 (a + b) - (m + p) then
    reach 4590 and -510, so that sat8 works on both sides; the chroma means see 0, 255 and both"""
    yy, xx = np.mgrid[0:h, 0:w]
    pat = ((((xx + 3) >> 1) ^ ((yy + 3) >> 1)) & 1) * 255
    cells = np.kron(rng.integers(0, 2, size=(h // 8 + 1, w // 8 + 1)), np.ones((8, 8), dtype=np.int64))[:h, :w]
    return np.where(cells == 1, pat, rng.integers(0, 256, size=(h, w))).astype(np.uint8)


def mk_frame(rng, geo, orc, fill=extreme):
    f = A.BorderedFrame(geo.w, geo.h, geo.fmt)
    for c in range(3):
        pw, ph = f.dims[c]
        f.plane(c)[:, :] = fill(rng, pw, ph)
    orc.orc_frame_extend(f.ptr())
    return f


def noise(rng, w, h):
    return rng.integers(0, 256, size=(h, w), dtype=np.uint8)


def smooth(rng, w, h):
    base = rng.integers(0, 256, size=(h // 8 + 2, w // 8 + 2)).astype(np.float64)
    return np.clip(np.kron(base, np.ones((8, 8)))[:h, :w] + rng.integers(-6, 7, size=(h, w)), 0, 255).astype(np.uint8)


def same_planes(geo, mv, tags, unp, got, want, what, fused=None):
    for c in range(3):
        msg = M.explain(geo, mv, tags, c, got.plane(c), want.plane(c), ~unp[c], what, fused)
        assert msg is None, msg


def same_raw(geo, unp, got, want, what):
    keep = M.raw_mask(geo, unp)
    A.assert_same("%s %s: frame bytes outside the planes' compared pixels" % (geo.name, what), got.raw()[keep], want.raw()[keep])


OP_CASES = M.op_cases()


@pytest.mark.parametrize("case", range(len(OP_CASES)), ids=["%s-%s-%d" % (g.name, r, s) for g, r, s in OP_CASES])
def test_operators(prod, orc, case):
    """dsvg_op_sub_pred / dsvg_op_add_pred = k_mc over the whole grid, all three bodies, at block sizes of the test's choosing"""
    geo, recipe, seed = OP_CASES[case]
    rng = np.random.default_rng(1000 + case)
    mv, tags = M.build_field(geo, recipe, seed)
    unp = M.unpinned_masks(geo, mv)
    mvp = mv.ctypes.data_as(C.POINTER(A.MV))
    meta = A.Meta(geo.w, geo.h, geo.fmt, 30, 1, 1, 1)
    prm = A.Params(C.pointer(meta), 1, 1, geo.bw, geo.bh, geo.nbh, geo.nbv)
    ref = mk_frame(rng, geo, orc)
    inp = mk_frame(rng, geo, orc, noise if case % 2 else extreme)
    ia, ib = A.BorderedFrame(geo.w, geo.h, geo.fmt), A.BorderedFrame(geo.w, geo.h, geo.fmt)
    ia.buf[:] = inp.buf
    ib.buf[:] = inp.buf
    # the prediction frames start zeroed: the last column / row of an odd clipped intra block is "untouched" in the reference
    # (orc_bmc.c:97-108) and zero in the product (k_bmc.hip:368), and on a zeroed frame the two coincide
    da, db = A.BorderedFrame(geo.w, geo.h, geo.fmt), A.BorderedFrame(geo.w, geo.h, geo.fmt)
    orc.orc_sub_pred(mvp, C.byref(prm), da.ptr(), ia.ptr(), ref.ptr())
    A.chk(prod, prod.dsvg_op_sub_pred(mvp, C.byref(prm), db.ptr(), ib.ptr(), ref.ptr()))
    same_planes(geo, mv, tags, unp, db, da, "sub_pred prediction")
    same_planes(geo, mv, tags, unp, ib, ia, "sub_pred residual")
    same_raw(geo, unp, db, da, "sub_pred prediction")
    same_raw(geo, unp, ib, ia, "sub_pred residual")
    # add_pred on the oracle's residual for both (the unpinned pixels of the product's own may differ); `out` zeroed for the same reason
    oa, ob = A.BorderedFrame(geo.w, geo.h, geo.fmt), A.BorderedFrame(geo.w, geo.h, geo.fmt)
    ic = A.BorderedFrame(geo.w, geo.h, geo.fmt)
    ic.buf[:] = ia.buf
    orc.orc_add_pred(mvp, C.byref(prm), ia.ptr(), oa.ptr(), ref.ptr())
    A.chk(prod, prod.dsvg_op_add_pred(mvp, C.byref(prm), ic.ptr(), ob.ptr(), ref.ptr()))
    same_planes(geo, mv, tags, unp, ob, oa, "add_pred")
    same_raw(geo, unp, ob, oa, "add_pred")
    A.assert_same("%s add_pred leaves the residual frame alone" % geo.name, ic.raw(), ia.raw())


# ---- context level: the decoder ------------------------------------------------------------------------------------------------------
import hashlib          # noqa: E402
import importlib        # noqa: E402
import json             # noqa: E402
import os               # noqa: E402
import subprocess       # noqa: E402
import sys              # noqa: E402

from _hzbits import plane_payload   # noqa: E402

CTX_CASES = M.ctx_cases()
CTX_IDS = [g.name for g, _, _ in CTX_CASES]
MAX_JOBS, N_RECON = 16, 8                   # a context with a second coding stream: a call of four P pictures forks
NJ = 4                                      # P pictures per call, each with a field of its own
QUANT = 120


def the_pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    L = m.lib()
    assert L.dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    L.dsvg_ctx_create.argtypes = [C.POINTER(C.c_void_p)] + [C.c_int] * 9
    L.dsvg_ctx_destroy.argtypes = [C.c_void_p]
    L.dsvg_ctx_destroy.restype = None
    L.dsvg_decode_pictures.argtypes = [C.c_void_p, C.c_int, C.POINTER(m.DecJob)]
    L.dsvg_download_recon.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.dsvg_download_recon_raw.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.dsvg_upload_recon_raw.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.dsvg_recon_border.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.dsvg_prof_kernel_name.restype = C.c_char_p
    L.dsvg_ctx_decoder_redone.restype = C.c_long
    L.dsvg_ctx_decoder_redone.argtypes = [C.c_void_p]
    return m


@pytest.fixture(scope="module")
def pkg():
    return the_pkg()


def extended_mask(geo, unp, orc):
    """bool over a frame's raw bytes: False where an unpinned pixel lies or is replicated into the border"""
    f = A.BorderedFrame(geo.w, geo.h, geo.fmt)
    for c in range(3):
        f.plane(c)[:, :] = unp[c]
    orc.orc_frame_extend(f.ptr())
    return f.raw() == 0


def new_ctx(L, geo, env, n_src, n_recon, max_jobs, out_slots, pyramid=0):
    """a context created with `env` set: a context reads its switches at creation"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    ctx = C.c_void_p(None)
    try:
        A.chk(L, L.dsvg_ctx_create(C.byref(ctx), 0, geo.w, geo.h, geo.fmt, pyramid, n_src, n_recon, max_jobs, out_slots))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return ctx


RESIDUALS = ("empty", "residual", "flagged")
QUANTS = {"empty": 120, "residual": 40, "flagged": 120}


class DecCase:
    """one context geometry: the reference picture, NJ + 1 built fields with their payloads, and the oracle's pictures composed as
    oracle/orc_dec.c:122-157 does: orc_decode_plane -> orc_inv_sbt(isP = 1) -> orc_add_pred -> orc_frame_extend.  Pictures 0 .. NJ - 1
    are one call (slot 0 -> slots 1 .. NJ); picture NJ is a call of its own that updates its reference in place (slot NJ + 1 -> NJ + 1).
    residual: three planes of an empty chain; a DC and a dozen symbols of +-1, +-2 at quantiser 40 (on the 0 / 255 cells of the reference
    the sum saturates); the same with symbols up to 4 at quantiser 120, which the int16 symbol path's range check flags, so that the
    call is decoded a second time from int32 coefficients (dsvg_ctx_decoder_redone)"""
    _cache = {}

    @classmethod
    def of(cls, orc, idx, residual):
        if (idx, residual) not in cls._cache:
            cls._cache[(idx, residual)] = cls(orc, idx, residual)
        return cls._cache[(idx, residual)]

    def __init__(self, orc, idx, residual):
        geo, recipe, seed = CTX_CASES[idx]
        self.geo, self.quant = geo, QUANTS[residual]
        rng = np.random.default_rng(7000 + idx)
        self.ref = mk_frame(rng, geo, orc)
        self.fields = [M.build_field(geo, recipe, seed + 100 * k) for k in range(NJ + 1)]
        self.unp = [M.unpinned_masks(geo, mv) for mv, _ in self.fields]
        self.keep = [extended_mask(geo, u, orc) for u in self.unp]
        self.st = [(rng.integers(0, 2, geo.nblk) | 2 * (mv["mode"] != 0)).astype(np.uint8) for mv, _ in self.fields]
        small = residual == "residual"
        self.pay = [[np.frombuffer(plane_payload(0, []) if residual == "empty" else
                                   plane_payload((5 - 4 * c) * (k + 1), M.residual_entries(geo, c, idx * 10 + k, small)), dtype=np.uint8).copy()
                     for c in range(3)] for k in range(NJ + 1)]
        meta = A.Meta(geo.w, geo.h, geo.fmt, 30, 1, 1, 1)
        prm = A.Params(C.pointer(meta), 1, 1, geo.bw, geo.bh, geo.nbh, geo.nbv)
        self.want = []
        for k in range(NJ + 1):
            resid = A.BorderedFrame(geo.w, geo.h, geo.fmt)
            for c in range(3):
                cw, ch = A.coef_dims(geo.w, geo.h, geo.fmt, c)
                co = np.zeros(cw * ch, dtype=np.int32)
                st = A.Stability(C.pointer(prm), A.u8p(self.st[k]), c, 1)
                buf = np.concatenate([self.pay[k][c], np.zeros(16, np.uint8)])
                orc.orc_decode_plane(A.u8p(buf), len(self.pay[k][c]), C.byref(A.Coefs(A.i32p(co), cw, ch)), self.quant, C.byref(st))
                orc.orc_inv_sbt(C.byref(resid.c.planes[c]), C.byref(A.Coefs(A.i32p(co), cw, ch)), self.quant, 1, c)
            out = A.BorderedFrame(geo.w, geo.h, geo.fmt)
            orc.orc_add_pred(self.fields[k][0].ctypes.data_as(C.POINTER(A.MV)), C.byref(prm), resid.ptr(), out.ptr(), self.ref.ptr())
            orc.orc_frame_extend(out.ptr())
            self.want.append(out)

    def job(self, pkg, k, ref, recon):
        return pkg.DecJob(ref, recon, self.quant, self.fields[k][0].ctypes.data, self.st[k].ctypes.data,
                          (C.c_void_p * 3)(*[a.ctypes.data for a in self.pay[k]]), (C.c_uint32 * 3)(*[len(a) for a in self.pay[k]]))

    def jobs(self, pkg):
        return (pkg.DecJob * NJ)(*[self.job(pkg, k, 0, 1 + k) for k in range(NJ)])

    def plan(self, pkg, switches=0):
        g = self.geo
        return pkg.decode_plan(g.w, g.h, g.fmt, N_RECON, MAX_JOBS, switches, False, 0, NJ, self.jobs(pkg))

    def decode(self, pkg, env=None, profiled=False):
        """-> (packed pictures, raw extended frames, launches of the first call's k_mc bracket or None, calls decoded twice after the
        first and after the second call) on a context of its own, created with `env` set (a context reads its switches at creation)"""
        L, g = pkg.lib(), self.geo
        ctx = new_ctx(L, g, env or {}, 1, N_RECON, MAX_JOBS, MAX_JOBS, pyramid=1)
        try:
            for slot in (0, NJ + 1):
                A.chk(L, L.dsvg_upload_recon_raw(ctx, slot, self.ref.raw().ctypes.data, g.total))
            n = None
            if profiled:
                kid = [L.dsvg_prof_kernel_name(i).decode() for i in range(L.dsvg_prof_kernels())].index("k_mc")
                A.chk(L, L.dsvg_prof_enable(ctx, 1 << kid))
                A.chk(L, L.dsvg_prof_reset(ctx))
            packed, raw, redone = [], [], []

            def download(slot):
                p = np.zeros(A.frame_bytes(g.w, g.h, g.fmt), dtype=np.uint8)
                A.chk(L, L.dsvg_download_recon(ctx, slot, p.ctypes.data))
                r = np.zeros(g.total, dtype=np.uint8)
                A.chk(L, L.dsvg_download_recon_raw(ctx, slot, r.ctypes.data, g.total))
                packed.append(p)
                raw.append(r)
                return L.dsvg_ctx_decoder_redone(ctx)
            A.chk(L, L.dsvg_decode_pictures(ctx, NJ, self.jobs(pkg)))
            for k in range(NJ):
                redone[:] = [download(1 + k)]
            if profiled:
                ms, cnt, by = C.c_double(0), C.c_long(0), C.c_double(0)
                A.chk(L, L.dsvg_prof_get(ctx, kid, C.byref(ms), C.byref(cnt), C.byref(by)))
                n = cnt.value
            A.chk(L, L.dsvg_decode_pictures(ctx, 1, (pkg.DecJob * 1)(self.job(pkg, NJ, NJ + 1, NJ + 1))))
            redone.append(download(NJ + 1))
            return packed, raw, n, redone
        finally:
            L.dsvg_ctx_destroy(ctx)

    def check(self, packed, raw, what, plan=None):
        """plan: the call's, where k_mc_patch ran (a mismatch then names the pixel's kernel)"""
        g = self.geo
        for k in range(NJ + 1):
            mv, tags = self.fields[k]
            fused = M.dec_kernel_of(g, mv, plan["ex0"], plan["ey0"]) if plan is not None and plan["mc"] == 2 else None
            got = A.BorderedFrame(g.w, g.h, g.fmt)
            got.load_planar(packed[k])
            same_planes(g, mv, tags, self.unp[k], got, self.want[k], "%s picture %d" % (what, k), fused)
            got.buf[got.GUARD:got.GUARD + g.total] = raw[k]
            same_planes(g, mv, tags, self.unp[k], got, self.want[k], "%s picture %d, extended frame" % (what, k), fused)
            A.assert_same("%s %s picture %d: extended frame" % (g.name, what, k), raw[k][self.keep[k]], self.want[k].raw()[self.keep[k]])

    def digest(self, packed, raw):
        """of the compared bytes alone (a child process reports it)"""
        h = hashlib.sha256()
        for k in range(NJ + 1):
            h.update(raw[k][self.keep[k]].tobytes())
            f = A.BorderedFrame(self.geo.w, self.geo.h, self.geo.fmt)
            f.load_planar(packed[k])
            for c in range(3):
                h.update(f.plane(c)[~self.unp[k][c]].tobytes())
        return h.hexdigest()


# every geometry with an empty chain and with a small residual; the flagged residual where the first call's second pass was seen
DEC_CASES = [(i, r) for i in range(len(CTX_CASES)) for r in RESIDUALS[:2]] + [(0, "flagged"), (2, "flagged")]


@pytest.mark.parametrize("idx,residual", DEC_CASES, ids=["%s-%s" % (CTX_IDS[i], r) for i, r in DEC_CASES])
def test_decoder(pkg, orc, idx, residual):
    """k_mc_patch plus k_mc by list (fused geometries) or k_mc over the grid: a call of four P pictures with the fork, profiled (no
    fork), without the prediction in place and without the fused kernels, and a picture that updates its reference in place -- all of
    them the oracle's pictures, also where the call is decoded a second time"""
    case = DecCase.of(orc, idx, residual)
    geo = case.geo
    plan = case.plan(pkg)
    assert plan["fork"] == 1 and plan["second_stream"] == 1 and plan["mc"] == (2 if geo.fusable() else 1)
    assert list(plan["inplace"]) == [1] * NJ
    if plan["mc"] == 2:
        # k_mc by list: exactly the blocks the classifier sends there, and some
        want = np.concatenate([k * geo.nblk + M.list_blocks(geo, case.fields[int(src)][0], plan["ex0"], plan["ey0"])
                               for k, src in enumerate(plan["order"])])
        assert plan["iln"] > 0 and plan["ilist"].tolist() == want.tolist()
    else:
        assert plan["iln"] == 0
    packed, raw, _, redone = case.decode(pkg)
    case.check(packed, raw, "forked", plan)
    # the first call is decoded twice where its symbols say so (the flagged residual: always; the small one: where scan regions share
    # cells, 250x130); the picture that updates its reference never is -- its second pass would predict from its first
    assert redone[0] == {"empty": 0, "flagged": 1}.get(residual, redone[0]) and redone[0] <= 1 and redone[1] == redone[0], \
        "calls decoded twice after the first and after the second call: %s" % redone
    assert case.plan(pkg, pkg.DEC_PROFILED)["fork"] == 0
    packed, raw, n, redone = case.decode(pkg, profiled=True)
    if not redone[0]:
        assert n == (1 if plan["mc"] == 1 else 1 + (plan["iln"] > 0)), "launches of the k_mc bracket"
    case.check(packed, raw, "profiled", plan)
    assert not case.plan(pkg, pkg.DEC_NO_INPLACE_PRED)["inplace"].any()
    packed, raw, _, redone = case.decode(pkg, env={"DSV1_NO_INPLACE_PRED": "1"})
    case.check(packed, raw, "DSV1_NO_INPLACE_PRED", plan)
    if geo.fusable():
        assert case.plan(pkg, pkg.DEC_NO_MC_FUSION)["mc"] == 1
        packed, raw, _, redone = case.decode(pkg, env={"DSV1_NO_MC_FUSION": "1"})
        case.check(packed, raw, "DSV1_NO_MC_FUSION")


def _fused_dec_cases():
    return [(i, r) for i, r in DEC_CASES if CTX_CASES[i][0].fusable()]


def _decoder_digests(orc, pkg):
    return {"%s-%s" % (CTX_IDS[i], r): DecCase.of(orc, i, r).digest(*DecCase.of(orc, i, r).decode(pkg)[:2]) for i, r in _fused_dec_cases()}


def test_decoder_without_the_patch_kernel(pkg, orc):
    """DSV1_NO_MC_PATCH is read once per process: a child process decodes every fused case under it (plain k_mc over the grid) and
    reports a digest of the compared bytes, which must be that of the oracle's pictures"""
    want = {}
    for i, r in _fused_dec_cases():
        case = DecCase.of(orc, i, r)
        assert case.plan(pkg, pkg.DEC_NO_MC_PATCH)["mc"] == 1
        want["%s-%s" % (CTX_IDS[i], r)] = case.digest([w.to_planar() for w in case.want], [w.raw() for w in case.want])
    env = dict(os.environ, DSV1_NO_MC_PATCH="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "decoder-digests"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    bad = sorted(k for k in want if got.get(k) != want[k])
    assert not bad and set(got) == set(want), "under DSV1_NO_MC_PATCH the compared bytes differ from the oracle's: %s" % bad


# ---- context level: the encoder ------------------------------------------------------------------------------------------------------
class PicOut(C.Structure):
    _fields_ = [("dc", C.c_int32 * 3), ("nruns", C.c_uint32 * 3), ("nbytes", C.c_uint32 * 3), ("payload", C.c_void_p * 3),
                ("rc_quant", C.c_int32), ("rc_pkt_len", C.c_uint32)]


def enc_bind(pkg):
    L = pkg.lib()
    L.dsvg_load_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.dsvg_code_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(pkg.PicJob)]
    L.dsvg_code_pictures.argtypes = [C.c_void_p, C.c_int, C.POINTER(pkg.PicJob)]
    L.dsvg_fetch_pictures.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(PicOut)]
    return L


def header_of(payload):
    """(dc, run count, the code chain) of a plane payload: SEG(DC), alignment, 32 bits, the chain, the end-of-plane byte 0x55
    (hzcc.c:449-476); dsvg_fetch_pictures hands the three over apart"""
    from _hzbits import BR
    r = BR(payload + b"\0" * 8)
    dc = r.ueg()
    if dc and r.bit():
        dc = -dc
    r.align()
    runs = r.bits(32)
    assert payload[-1] == 0x55
    return dc, runs, payload[r.pos >> 3:-1]


def oracle_code(orc, geo, src, ref, mv, stable, quant):
    """one picture as oracle/orc_enc.c:425-460 codes it: orc_frame_copy -> orc_sub_pred (P) -> per plane orc_fwd_sbt / orc_encode_plane /
    orc_inv_sbt -> orc_frame_add (P).  src, ref: extended frames (ref None: an I picture).  -> ([(dc, runs, payload)] x 3, reconstruction).
    The prediction frame starts zeroed, as in the operator test."""
    isP = int(ref is not None)
    meta = A.Meta(geo.w, geo.h, geo.fmt, 30, 1, 1, 1)
    prm = A.Params(C.pointer(meta), 1, isP, geo.bw, geo.bh, geo.nbh, geo.nbv)
    xf, pred = A.BorderedFrame(geo.w, geo.h, geo.fmt), A.BorderedFrame(geo.w, geo.h, geo.fmt)
    xf.buf[:] = src.buf
    if isP:
        orc.orc_sub_pred(mv.ctypes.data_as(C.POINTER(A.MV)), C.byref(prm), pred.ptr(), xf.ptr(), ref.ptr())
    planes = []
    for c in range(3):
        cw, ch = A.coef_dims(geo.w, geo.h, geo.fmt, c)
        co = np.zeros(cw * ch, dtype=np.int32)
        cf = A.Coefs(A.i32p(co), cw, ch)
        st = A.Stability(C.pointer(prm), A.u8p(stable), c, isP)
        buf = np.zeros(cw * ch * 8 + 64, dtype=np.uint8)
        bs = A.BS(A.u8p(buf), 0)
        orc.orc_fwd_sbt(C.byref(xf.c.planes[c]), C.byref(cf), isP)
        orc.orc_encode_plane(C.byref(bs), C.byref(cf), quant, C.byref(st))
        plen = int.from_bytes(buf[:4].tobytes(), "big")
        pay = buf[4:4 + plen].tobytes()
        planes.append(header_of(pay))
        orc.orc_inv_sbt(C.byref(xf.c.planes[c]), C.byref(cf), quant, isP, c)
    if isP:
        orc.orc_frame_add(xf.ptr(), pred.ptr())
    return planes, xf


def true_reach(mv):
    """dsvg_pic_job.mv_reach: min / max of mv.x >> 1 and mv.y >> 1 over the inter blocks, each taken with 0"""
    m = mv[mv["mode"] == 0]
    x, y = m["x"].astype(np.int32) >> 1, m["y"].astype(np.int32) >> 1
    return (C.c_short * 4)(min(0, int(x.min(initial=0))), max(0, int(x.max(initial=0))), min(0, int(y.min(initial=0))), max(0, int(y.max(initial=0))))


def fetch(L, ctx, n):
    slots = (C.c_int * n)(*range(n))
    outs = (PicOut * n)()
    A.chk(L, L.dsvg_fetch_pictures(ctx, n, slots, outs))
    return [[(o.dc[p], o.nruns[p], C.string_at(o.payload[p], o.nbytes[p])) for p in range(3)] for o in outs]


def same_coded(geo, what, got, want):
    for p in range(3):
        assert got[p][:2] == want[p][:2], "%s %s plane %d: dc, runs %s, the oracle's %s" % (geo.name, what, p, got[p][:2], want[p][:2])
        if got[p][2] != want[p][2]:
            n = min(len(got[p][2]), len(want[p][2]))
            first = next((i for i in range(n) if got[p][2][i] != want[p][2][i]), n)
            raise AssertionError("%s %s plane %d: payload differs from the oracle's at byte %d (%d against %d bytes)" % (
                geo.name, what, p, first, len(got[p][2]), len(want[p][2])))


def recon_of(L, ctx, geo, slot):
    p = np.zeros(A.frame_bytes(geo.w, geo.h, geo.fmt), dtype=np.uint8)
    A.chk(L, L.dsvg_download_recon(ctx, slot, p.ctypes.data))
    f = A.BorderedFrame(geo.w, geo.h, geo.fmt)
    f.load_planar(p)
    return f


ENC_QUANTS = (16, 300)


@pytest.mark.parametrize("idx", range(len(CTX_CASES)), ids=CTX_IDS)
def test_encoder(pkg, orc, idx):
    """k_fwd_mc_fast, k_fwd_mc_pix and k_mc by list (fused geometries; plain k_mc under DSV1_NO_MC_FUSION and on 384x240): one call of
    two P pictures -- quantiser 16 with intra blocks, quantiser 300 without -- from an uploaded reference, with the job's hints unset
    and set.  No pixel of an encoder field is unpinned: a coded plane depends on every pixel of the prediction."""
    geo = CTX_CASES[idx][0]
    L = enc_bind(pkg)
    rng = np.random.default_rng(9000 + idx)
    ref = mk_frame(rng, geo, orc)
    srcs = [mk_frame(rng, geo, orc, smooth), mk_frame(rng, geo, orc)]
    fields = [M.build_field(geo, "full-pinned", 60 + idx), M.build_field(geo, "inter-pinned", 80 + idx)]
    stables = [rng.integers(0, 4, geo.nblk).astype(np.uint8) for _ in range(2)]
    assert not any(u.any() for mv, _ in fields for u in M.unpinned_masks(geo, mv))
    want = [oracle_code(orc, geo, srcs[k], ref, fields[k][0], stables[k], ENC_QUANTS[k]) for k in range(2)]
    yuv = np.concatenate([s.to_planar() for s in srcs])
    got = {}
    for env in ({}, {"DSV1_NO_MC_FUSION": "1"}) if geo.fusable() else ({},):
        for hints in (0, 1):
            jobs = (pkg.PicJob * 2)()
            for k in range(2):
                mv = fields[k][0]
                jobs[k] = pkg.PicJob(k, 0, 1 + k, ENC_QUANTS[k], mv.ctypes.data, stables[k].ctypes.data, k, int(hints and k == 1), hints,
                                     true_reach(mv) if hints else (C.c_short * 4)(), 0)
            sw = pkg.BATCH_NO_MC_FUSION if env else 0
            plan = pkg.code_batch_plan(geo.w, geo.h, geo.fmt, 3, 2, 2, 2, 2, sw, 1, 2, jobs)
            assert plan["mc_fused"] == int(geo.fusable() and not env)
            if plan["mc_fused"]:
                # k_mc by list: the intra blocks of the first picture, relative to the first P job of its group's launch; none of the second
                intra = np.nonzero(fields[0][0]["mode"] != 0)[0]
                assert plan["icnt"].sum() == intra.size > 0 and plan["ilist"].tolist() == intra.tolist()
            what = "%s hints %d" % ("DSV1_NO_MC_FUSION" if env else "fused" if geo.fusable() else "plain", hints)
            ctx = new_ctx(L, geo, env, 2, 3, 2, 2)
            try:
                A.chk(L, L.dsvg_load_frames(ctx, 0, 2, yuv.ctypes.data, 0, 1))
                A.chk(L, L.dsvg_upload_recon_raw(ctx, 0, ref.raw().ctypes.data, geo.total))
                A.chk(L, L.dsvg_code_pictures(ctx, 2, jobs))
                coded = fetch(L, ctx, 2)
                for k in range(2):
                    # the reconstruction first: a mismatch there names the pixel, its block's path class and its kernel
                    mv, tags = fields[k]
                    same_planes(geo, mv, tags, [np.zeros((d[1], d[0]), dtype=bool) for d in geo.dims], recon_of(L, ctx, geo, 1 + k), want[k][1],
                                "%s reconstruction %d" % (what, k), M.enc_kernel_of(geo, mv) if plan["mc_fused"] else None)
                    same_coded(geo, "%s picture %d" % (what, k), coded[k], want[k][0])
                got[what] = coded
            finally:
                L.dsvg_ctx_destroy(ctx)
    assert all(v == got[next(iter(got))] for v in got.values()), "the hints or the switch change the coded bytes"


def tap_need(geo, mv):
    """how far the taps of the field's inter blocks reach beyond the picture: [left, right, above, below] x (luma, chroma), in pixels"""
    need = [0] * 8
    for c in (0, 1):
        pw, ph = geo.dims[c]
        lo, hi = (1, 2) if c == 0 else (0, 1)
        for k in np.nonzero(mv["mode"] == 0)[0]:
            i, j = int(k) % geo.nbh, int(k) // geo.nbh
            b = geo.block(c, i, j)
            if b is None:
                continue
            wx, wy, xh, yh, _, _ = M.placed(geo, c, i, j, mv[k]["x"], mv[k]["y"])
            n = need[4 * c:4 * c + 4]
            n = [max(n[0], (lo if xh else 0) - wx), max(n[1], wx + b[2] - 1 + (hi if xh else 0) - (pw - 1)),
                 max(n[2], (lo if yh else 0) - wy), max(n[3], wy + b[3] - 1 + (hi if yh else 0) - (ph - 1))]
            need[4 * c:4 * c + 4] = n
    return need


@pytest.mark.parametrize("recipe", ["zero", "reach5", "beyond"])
@pytest.mark.parametrize("idx", [0, 1], ids=CTX_IDS[:2])
def test_lazy_border(pkg, orc, idx, recipe):
    """dsvg_code_batch of two steps, I then P from the I picture's reconstruction with border_hint = 1: the border written covers what
    the field reads, and the P picture is that of DSV1_NO_LAZY_BORDER and of the oracle"""
    geo = CTX_CASES[idx][0]
    L = enc_bind(pkg)
    rng = np.random.default_rng(9500 + idx)
    srcs = [mk_frame(rng, geo, orc, noise), mk_frame(rng, geo, orc, noise)]
    mv, tags = M.build_field(geo, recipe, 90 + idx)
    assert not any(u.any() for u in M.unpinned_masks(geo, mv))
    stables = [rng.integers(0, 4, geo.nblk).astype(np.uint8) for _ in range(2)]
    wantI = oracle_code(orc, geo, srcs[0], None, None, stables[0], 40)
    orc.orc_frame_extend(wantI[1].ptr())
    wantP = oracle_code(orc, geo, srcs[1], wantI[1], mv, stables[1], 40)
    yuv = np.concatenate([s.to_planar() for s in srcs])
    need = tap_need(geo, mv)
    out = {}
    for env in ({}, {"DSV1_NO_LAZY_BORDER": "1"}):
        jobs = (pkg.PicJob * 2)()
        jobs[0] = pkg.PicJob(0, -1, 0, 40, None, stables[0].ctypes.data, 0, 0, 0, (C.c_short * 4)(), 1)
        jobs[1] = pkg.PicJob(1, 0, 1, 40, mv.ctypes.data, stables[1].ctypes.data, 1, 0, 0, (C.c_short * 4)(), 1)
        ctx = new_ctx(L, geo, env, 2, 2, 1, 2)
        try:
            A.chk(L, L.dsvg_load_frames(ctx, 0, 2, yuv.ctypes.data, 0, 1))
            A.chk(L, L.dsvg_code_batch(ctx, 2, 1, jobs))
            border = np.zeros(8, dtype=np.int16)
            A.chk(L, L.dsvg_recon_border(ctx, 0, border.ctypes.data))
            coded = fetch(L, ctx, 2)
            what = "%s %s" % (recipe, "DSV1_NO_LAZY_BORDER" if env else "lazy")
            for i in range(8):
                assert border[i] >= min(64, need[i]), \
                    "%s %s: border %s of the I picture's slot, the field's taps reach %s" % (geo.name, what, border.tolist(), need)
            if env:
                assert (border == 64).all()
            elif recipe == "zero":
                assert (border < 64).all(), "a zero field needs no whole border: %s" % border.tolist()
            elif recipe == "beyond":
                assert (border == 64).all()
            same_coded(geo, what + " I picture", coded[0], wantI[0])
            same_coded(geo, what + " P picture", coded[1], wantP[0])
            none = [np.zeros((d[1], d[0]), dtype=bool) for d in geo.dims]
            same_planes(geo, mv, tags, none, recon_of(L, ctx, geo, 1), wantP[1], what + " P reconstruction")
            out[bool(env)] = coded
        finally:
            L.dsvg_ctx_destroy(ctx)
    assert out[False] == out[True], "the lazy border changes the coded bytes"


if __name__ == "__main__" and sys.argv[1:] == ["decoder-digests"]:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps(_decoder_digests(A.load_orc(), the_pkg()), sort_keys=True))
