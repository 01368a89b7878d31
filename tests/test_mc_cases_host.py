"""The case table of tests/mc_cases.py, checked on the CPU: every built field respects the two bounds of the reference, the unpinned
mask is what the oracle itself shows when the bytes around a frame change, the float reciprocal of k_fwd_mc_fast lands every patch in
its block, and the ledger -- every path class the table is meant to reach is reached."""
import collections
import ctypes as C

import numpy as np
import pytest

import _cabi as A
import mc_cases as M

CASES = M.all_cases()
IDS = ["%s-%s-%d" % (g.name, r, s) for g, r, s in CASES]


@pytest.fixture(scope="module")
def fields():
    return [(g, r, s) + M.build_field(g, r, s) for g, r, s in CASES]


def test_fields_keep_the_reference_defined(fields):
    for geo, recipe, seed, mv, tags in fields:
        # no division by zero: a partial submask only where every plane's clipped block is at least 2 x 2
        for k in np.nonzero((mv["mode"] != 0) & (mv["submask"] != 0xF))[0]:
            for c in range(3):
                b = geo.block(c, int(k) % geo.nbh, int(k) // geo.nbh)
                assert b is None or (b[2] >= 2 and b[3] >= 2), (geo.name, int(k), c)
        assert ((mv["mode"] == 0) | ((mv["submask"] >= 1) & (mv["submask"] <= 15))).all()
        # unpinned pixels: first block row of luma, last block row of V, under a tenth of the picture
        unp = M.unpinned_masks(geo, mv)
        assert not unp[1].any(), geo.name
        assert not unp[0][geo.bh:].any(), geo.name
        assert not unp[2][:(geo.nbv - 1) * (geo.bh >> geo.vs)].any(), geo.name
        total = sum(u.size for u in unp)
        assert sum(int(u.sum()) for u in unp) * 10 < total, geo.name
        if M.RECIPES[recipe]["pinned"]:
            assert not any(u.any() for u in unp), geo.name


def _frames(geo, seed, junk):
    """a reference frame with `junk` in every byte around its allocation"""
    rng = np.random.default_rng(seed)
    f = A.BorderedFrame(geo.w, geo.h, geo.fmt)
    for c in range(3):
        f.plane(c)[:, :] = rng.integers(0, 256, f.plane(c).shape, dtype=np.uint8)
    A.load_orc().orc_frame_extend(f.ptr())
    f.buf[:f.GUARD] = junk
    f.buf[f.GUARD + f.total:] = junk
    return f


@pytest.mark.parametrize("case", range(0, len(M.op_cases()), 5))
def test_unpinned_is_what_the_bytes_around_a_frame_decide(orc, case):
    """the oracle's prediction with 0x00 and with 0xFF around the reference frame: the same at every pinned pixel, and the unpinned
    ones are no wider than needed -- each row of them differs somewhere between the two"""
    geo, recipe, seed = M.op_cases()[case]
    mv, tags = M.build_field(geo, recipe, seed)
    unp = M.unpinned_masks(geo, mv)
    meta = A.Meta(geo.w, geo.h, geo.fmt, 30, 1, 1, 1)
    prm = A.Params(C.pointer(meta), 1, 1, geo.bw, geo.bh, geo.nbh, geo.nbv)
    out = []
    for junk in (0, 255):
        ref = _frames(geo, seed, junk)
        d, i = A.BorderedFrame(geo.w, geo.h, geo.fmt), A.BorderedFrame(geo.w, geo.h, geo.fmt)
        orc.orc_sub_pred(mv.ctypes.data_as(C.POINTER(A.MV)), C.byref(prm), d.ptr(), i.ptr(), ref.ptr())
        out.append(d)
    for c in range(3):
        a, b = out[0].plane(c), out[1].plane(c)
        msg = M.explain(geo, mv, tags, c, a, b, ~unp[c], "junk 0 against junk 255")
        assert msg is None, msg
        rows = np.nonzero(unp[c].any(axis=1))[0]
        assert all((a[r] != b[r]).any() for r in rows), (geo.name, c)


def test_float_reciprocal_finds_every_patch_its_block():
    """k_sbt.hip:917-918: (int)((I + 0.5f) * rcp(bw >> 3)) against I // (bw >> 3) for every patch column and row of every fused case
    geometry, and for every block width the fused path admits up to the widest picture, with the reciprocal correctly rounded and one
    ulp off either way (v_rcp_f32 is allowed one)"""
    seen = set()
    for geo, _, _ in CASES:
        if not geo.fusable():
            continue
        for c in (0, 1):
            bw, bh = geo.blk(c)
            pw, ph = geo.dims[c]
            seen.add((bw >> 3, -(-pw // 8)))
            seen.add((bh >> 3, -(-ph // 8)))
    for n in (1, 2, 3, 4, 6, 8):
        seen.add((n, 2048))
    assert max(cnt for _, cnt in seen) >= 1100
    for n, cnt in sorted(seen):
        I = np.arange(cnt)
        for ulp in (0, -1, 1):
            got = M.fast_block_index(I, n, ulp)
            bad = np.nonzero(got != I // n)[0]
            assert bad.size == 0, "patch %d of blocks %d patches wide lands in block %d (reciprocal %+d ulp)" % (bad[0], n, got[bad[0]], ulp)


# ---- the ledger ---------------------------------------------------------------------------------------------------------------------
def wanted_classes():
    want = []
    for kind in ("copy", "lumaH", "chromaH"):
        want += ["row-%s-shb%d" % (kind, s) for s in range(4)]
    want += ["window-V", "window-HV", "window-chroma-V", "window-chroma-HV"]
    for w in (16, 32, 64):
        want += ["intra-lean-w%d-%s" % (w, p) for p in ("all", "partial")]
    for shape in ("whole", "clipped-even", "clipped-odd"):
        want += ["intra-window-%s-%s" % (shape, p) for p in ("all", "partial")]
    for s in range(1, 16):
        want += ["lean-sub%d" % s, "window-sub%d" % s]
    for kind in ("luma", "chroma"):
        for side in "LRTB":
            want += ["clamp-%s-%s-%s" % (kind, side, r) for r in ("in", "at", "out", "far")]
    return want


# classes no geometry of the table can reach, with the reason (at most five)
UNREACHABLE = {}


def ledger(fields):
    """class -> count of (block, plane); lean widths per plane kind as 'intra-lean-w<n>/luma' / '/chroma'"""
    n = collections.Counter()
    for geo, recipe, seed, mv, tags in fields:
        for c in range(3):
            for t in tags[c]:
                for name in t or ():
                    n[name] += 1
                    if name.startswith("intra-lean-w"):
                        n[name.rsplit("-", 1)[0] + ("/luma" if c == 0 else "/chroma")] += 1
    return n


def fused_ledger(n):
    """fast / pix / list of the encoder, patch / list of the decoder and (ex0, ey0) at and inside the grid's edge, over the context cases,
    from the product's own plans (device-free)"""
    import importlib
    pkg = importlib.import_module("digital-subband-video-1_amd")
    for geo, recipe, seed in M.ctx_cases():
        if not geo.fusable():
            continue
        mv, _ = M.build_field(geo, recipe, seed)
        st = np.zeros(geo.nblk, dtype=np.uint8)
        pay = np.zeros(16, dtype=np.uint8)
        job = (pkg.DecJob * 1)(pkg.DecJob(0, 1, 100, mv.ctypes.data, st.ctypes.data, (C.c_void_p * 3)(*[pay.ctypes.data] * 3), (C.c_uint32 * 3)(8, 8, 8)))
        p = pkg.decode_plan(geo.w, geo.h, geo.fmt, 2, 1, 0, False, 0, 1, job)
        assert p["mc"] == 2 and p["ilist"].tolist() == M.list_blocks(geo, mv, p["ex0"], p["ey0"]).tolist(), geo.name
        n["dec-list"] += p["iln"]
        n["dec-patch"] += geo.nblk - p["iln"]
        n["ex0-at-edge" if p["ex0"] == geo.nbh else "ex0-inside"] += 1
        n["ey0-at-edge" if p["ey0"] == geo.nbv else "ey0-inside"] += 1
        pj = (pkg.PicJob * 1)(pkg.PicJob(0, 0, 1, 100, mv.ctypes.data, st.ctypes.data, 0, 0, 0, (C.c_short * 4)(), 0))
        b = pkg.code_batch_plan(geo.w, geo.h, geo.fmt, 2, 1, 1, 1, 2, 0, 1, 1, pj)
        assert b["mc_fused"] == 1 and b["ilist"].tolist() == np.nonzero(mv["mode"] != 0)[0].tolist(), geo.name
        for k, v in M.enc_paths(geo, mv).items():
            n["enc-" + k] += v
    return n


FUSED = ["enc-fast", "enc-pix", "enc-list", "dec-patch", "dec-list", "ex0-at-edge", "ex0-inside", "ey0-at-edge", "ey0-inside"]


def test_ledger_every_path_class_is_reached(fields):
    n = fused_ledger(ledger(fields))
    want = wanted_classes() + ["intra-lean-w%d/%s" % (w, k) for w in (16, 32, 64) for k in ("luma", "chroma")] + FUSED
    assert len(UNREACHABLE) <= 5
    missing = [k for k in want if not n[k] and k not in UNREACHABLE]
    assert not missing, "the case table reaches no block of: %s" % ", ".join(missing)
    assert not [k for k in UNREACHABLE if n[k]], "listed as unreachable, but reached"
