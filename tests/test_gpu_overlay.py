"""The overlay pass on the GPU (include/dsv1_api.h, Overlays; csrc/k_overlay.hip) against tests/_overlay.py: the standalone call on host
and device memory between sentinel bytes, and the sessions -- whose streams are byte for byte those of the same session fed the
numpy-composited clips, and the oracle's.  Every comparison is exact."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _chroma as CH
import _overlay as OV
import _pixfmt as PF
import _reframe as R
import _scale as Z

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
CRF = dict(gop=4, rc_mode_cli=1, scd=1)
S, F = 2, 4
W, H = 70, 50                                             # the sessions' geometry
CANVASES = [(70, 50), (33, 17), (96, 64)]                 # 33 x 17: odd, the chroma edge samples cover one luma sample


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


class DevMem:
    """device memory through a small batch's context"""

    def __init__(self, pkg):
        self.b = pkg.Batch(pkg.make_encoder_cfg(64, 64, A.SUBSAMP_420), 1, 1)
        self.L = self.b.L

    def alloc(self, arr):
        return self.b.upload(arr)

    def read(self, p, nbytes):
        self.b.sync()
        out = np.zeros(nbytes, dtype=np.uint8)
        assert self.L.dsvg_dev_download(self.b.ctx, out.ctypes.data, p, nbytes) == 0
        return out

    def close(self):
        self.b.close()


@pytest.fixture(scope="module")
def mem(pkg):
    m = DevMem(pkg)
    yield m
    m.close()


def po(pkg, o):
    """the package's Overlay of a tests/_overlay.py placement"""
    return pkg.Overlay(o["planes"], o["w"], o["h"], o["x"], o["y"], o["source"], o["t0"], o["dur"], o["fade_in"], o["fade_out"], o["opacity"],
                       o["reserved"])


def pos(pkg, ovs):
    return [po(pkg, o) for o in ovs]


def noise(n, w, h, fmt, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, A.frame_bytes(w, h, fmt)), dtype=np.uint8)


# ---- the standalone call ----------------------------------------------------------------------------------------------------------
def check_clip(pkg, mem, fmt, w, h, n, ovs, t_first, tag, host=True):
    """host memory, then device memory at two alignments with sentinel bytes on both sides: equal to numpy, nothing written outside"""
    fb = A.frame_bytes(w, h, fmt)
    src = noise(n, w, h, fmt, 0x0E1 + fmt + w + n)
    want = OV.composite(src, w, h, fmt, ovs, t_first)
    tag = "%s 0x%x %dx%d n=%d t=%d" % (tag, fmt, w, h, n, t_first)
    lst = pos(pkg, ovs)
    if host:
        A.assert_same("host " + tag, pkg.overlay_clip(src, w, h, fmt, lst, t_first=t_first), want)
    for off in (256, 259):
        big = np.full(off + n * fb + 64, 0x99, dtype=np.uint8)
        big[off:off + n * fb] = src.reshape(-1)
        p = mem.alloc(big)
        pkg.overlay_clip(C.c_void_p(p.value + off), w, h, fmt, lst, t_first=t_first, n=n)
        after = mem.read(p, big.size)
        assert (after[:off] == 0x99).all() and (after[off + n * fb:] == 0x99).all(), "written outside the clip (device) " + tag
        A.assert_same("device offset %d %s" % (off, tag), after[off:off + n * fb].reshape(want.shape), want)
    return src, want


def aligned_down(v, s):
    return v >> s << s


def single_overlays(w, h, fmt):
    """(name, placement without a bitmap) for one canvas: 1 x 1 at the origin; 5 x 3; 33 x 17 in the middle at an aligned x that is no
    multiple of 4 (4:1:1 has none: no multiple of 16 there); one that ends exactly at the right and bottom edges; the whole canvas"""
    hs, vs = A.hshift(fmt), A.vshift(fmt)
    out = [("1x1", dict(w=1, h=1, x=0, y=0)), ("5x3", dict(w=5, h=3, x=aligned_down(w // 3, hs), y=aligned_down(h // 2, vs)))]
    if w >= 33 + 24 and h >= 17 + 16:
        x = {0: 17, 1: 18, 2: 20}[hs]
        assert x % (1 << hs) == 0 and x % (16 if hs == 2 else 4)
        out.append(("33x17", dict(w=33, h=17, x=x, y=aligned_down(13, vs))))
    ex, ey = aligned_down(w - 9, hs), aligned_down(h - 6, vs)
    out.append(("edge", dict(w=w - ex, h=h - ey, x=ex, y=ey)))
    out.append(("whole", dict(w=w, h=h, x=0, y=0)))
    return out


@pytest.mark.parametrize("canvas", CANVASES, ids=["%dx%d" % c for c in CANVASES])
@pytest.mark.parametrize("fmt", OV.FORMATS, ids=["0x%x" % f for f in OV.FORMATS])
def test_one_overlay_equals_numpy(pkg, mem, fmt, canvas):
    w, h = canvas
    alphas = ["random", 0, 255]
    # op 256, 128 and 1 through the fade: opacity 256 and a fade-in of 255 pictures seen at its end, its middle and its first picture
    times = [(255, 256), (127, 128), (0, 1)]
    for k, (name, geo) in enumerate(single_overlays(w, h, fmt)):
        for j in range(3):
            alpha, (t, op) = alphas[(k + j) % 3], times[(k + 2 * j) % 3]
            o = OV.ov(OV.bitmap(geo["w"], geo["h"], fmt, 31 * k + j, alpha), **geo, source=(-1, 0)[j & 1], t0=1000, dur=0, fade_in=255)
            assert OV.valid(o, w, h, fmt, 1) and OV.opacity_at(o, 1000 + t) == op
            src, want = check_clip(pkg, mem, fmt, w, h, 1, [o], 1000 + t, "%s alpha %s op %d" % (name, alpha, op), host=j == 0)
            if alpha == 0:
                assert np.array_equal(src, want)
            elif op == 256 and geo["w"] * geo["h"] >= 15:
                assert not np.array_equal(src, want)
    # op 0: before the first picture nothing is touched
    o = OV.ov(OV.bitmap(w, h, fmt, 5, 255), w, h, t0=1000)
    src, want = check_clip(pkg, mem, fmt, w, h, 1, [o], 999, "not yet")
    assert np.array_equal(src, want)
    src, want = check_clip(pkg, mem, fmt, w, h, 1, [o], 1000, "opaque whole canvas")
    assert np.array_equal(want[0], o["planes"][:A.frame_bytes(w, h, fmt)])           # alpha 255 at op 256 returns the bitmap


def fade_list(w, h, fmt, t):
    """five overlays whose fades ramp inside pictures t .. t + 4, overlapping each other"""
    hs, vs = A.hshift(fmt), A.vshift(fmt)
    ax, ay = lambda v: aligned_down(v, hs), lambda v: aligned_down(v, vs)
    return [OV.ov(OV.bitmap(33, 17, fmt, 1), 33, 17, x=ax(20), y=ay(13), t0=t + 1, dur=0, fade_in=3),                # op 0, 64, 128, 192, 256
            OV.ov(OV.bitmap(21, 9, fmt, 2), 21, 9, x=ax(8), y=ay(6), t0=t - 6, dur=9, fade_out=3, opacity=255),      # ... fades out and ends
            OV.ov(OV.bitmap(w, 5, fmt, 3), w, 5, x=0, y=ay(h - 11), t0=t - 1, dur=0, opacity=1),                     # op 1 throughout
            OV.ov(OV.bitmap(9, 9, fmt, 4, 255), 9, 9, x=ax(24), y=ay(16), t0=t, dur=0, opacity=0),                   # never visible
            OV.ov(OV.bitmap(15, 11, fmt, 5, 255), 15, 11, x=ax(28), y=ay(10), t0=t + 2, dur=2, fade_in=1, fade_out=1, opacity=200)]


@pytest.mark.parametrize("fmt", OV.FORMATS, ids=["0x%x" % f for f in OV.FORMATS])
def test_fades_inside_a_clip_of_five(pkg, mem, fmt):
    w, h, t = 70, 50, 40
    ovs = fade_list(w, h, fmt, t)
    assert [OV.opacity_at(ovs[0], t + i) for i in range(5)] == [0, 64, 128, 192, 256]
    assert [OV.opacity_at(ovs[1], t + i) for i in range(5)] == [191, 128, 64, 0, 0]
    assert OV.plan(ovs, 1, 5, [t])[1] >= 2
    src, want = check_clip(pkg, mem, fmt, w, h, 5, ovs, t, "fades")
    assert all(not np.array_equal(src[i], want[i]) for i in range(5))
    # one frame far behind the ramps: the steady state
    check_clip(pkg, mem, fmt, w, h, 1, ovs, t + 100, "steady")


@pytest.mark.parametrize("fmt", OV.FORMATS, ids=["0x%x" % f for f in OV.FORMATS])
def test_order_matters_where_two_overlap(pkg, mem, fmt):
    w, h = 70, 50
    hs, vs = A.hshift(fmt), A.vshift(fmt)
    a = OV.ov(OV.bitmap(30, 20, fmt, 11), 30, 20, x=aligned_down(8, hs), y=aligned_down(6, vs), opacity=230)
    b = OV.ov(OV.bitmap(25, 21, fmt, 12), 25, 21, x=aligned_down(24, hs), y=aligned_down(15, vs), opacity=256)
    assert OV.intersects(a, b) and OV.plan([a, b], 1, 1, [0])[1] == 2
    _, ab = check_clip(pkg, mem, fmt, w, h, 1, [a, b], 0, "a under b")
    _, ba = check_clip(pkg, mem, fmt, w, h, 1, [b, a], 0, "b under a")
    assert not np.array_equal(ab, ba)


@pytest.mark.parametrize("fmt", OV.FORMATS, ids=["0x%x" % f for f in OV.FORMATS])
def test_touching_overlays_of_one_layer_in_one_launch(pkg, mem, fmt):
    """neighbours in luma and in chroma, odd sizes, opaque: a kernel that wrote a byte next to its rectangle -- even the value it read
    -- would race with the neighbour; every byte outside the union is unchanged"""
    w, h = 70, 50
    hs, vs = A.hshift(fmt), A.vshift(fmt)
    al, av = 1 << hs, 1 << vs
    x0, y0 = 3 * al, 3 * av
    w0, h0 = 5 * al, 5 * av
    ovs = [OV.ov(OV.bitmap(w0, h0, fmt, 21, 255), w0, h0, x=x0, y=y0),
           OV.ov(OV.bitmap(17, h0, fmt, 22, 255), 17, h0, x=x0 + w0, y=y0),                     # right of it, touching
           OV.ov(OV.bitmap(w0 + 17, 7, fmt, 23, 255), w0 + 17, 7, x=x0, y=y0 + h0),              # below both, touching
           OV.ov(OV.bitmap(al + 1, 3, fmt, 24, 255), al + 1, 3, x=x0 - 2 * al, y=y0),            # left of the first, odd width
           OV.ov(OV.bitmap(3, 3, fmt, 25, 255), 3, 3, x=x0 + w0 + 17 + (-(x0 + w0 + 17)) % al, y=y0)]
    assert all(OV.valid(o, w, h, fmt, 1) for o in ovs)
    items, layers = OV.plan(ovs, 1, 2, [0])
    assert layers == 1 and len(items) == 10
    src, want = check_clip(pkg, mem, fmt, w, h, 2, ovs, 0, "touching")
    luma = np.zeros((h, w), dtype=bool)
    for o in ovs:
        luma[o["y"]:o["y"] + o["h"], o["x"]:o["x"] + o["w"]] = True
    got = pkg.overlay_clip(src, w, h, fmt, pos(pkg, ovs))
    for i in range(2):
        assert np.array_equal(got[i][:w * h].reshape(h, w)[~luma], src[i][:w * h].reshape(h, w)[~luma])
        for o in ovs:                                     # opaque at op 256: the bitmap's luma itself
            assert np.array_equal(got[i][:w * h].reshape(h, w)[o["y"]:o["y"] + o["h"], o["x"]:o["x"] + o["w"]], OV.planes_of(o, fmt)[0])


def test_many_items_many_tiles(pkg, mem):
    """a list long enough for several hundred table entries, on a canvas whose rows span several tiles"""
    fmt, w, h, n = A.SUBSAMP_420, 640, 96, 3
    rng = np.random.default_rng(9)
    ovs = [OV.ov(OV.bitmap(640, 96, fmt, 1), 640, 96, opacity=77)]
    for k in range(60):
        ow, oh = int(rng.integers(1, 40)), int(rng.integers(1, 20))
        ovs.append(OV.ov(OV.bitmap(ow, oh, fmt, 100 + k), ow, oh, x=aligned_down(int(rng.integers(0, w - ow)), 1),
                         y=aligned_down(int(rng.integers(0, h - oh)), 1), t0=int(rng.integers(-2, 2)), dur=3 * int(rng.integers(0, 2)),
                         fade_in=int(rng.integers(0, 3)), opacity=int(rng.integers(1, 257))))
    assert all(OV.valid(o, w, h, fmt, 1) for o in ovs)
    assert len(OV.plan(ovs, 1, n, [0])[0]) > 100
    check_clip(pkg, mem, fmt, w, h, n, ovs, 0, "many")


# ---- sessions ------------------------------------------------------------------------------------------------------------------
_cache = {}


def sources(fmt, w, h, n=2 * F):
    key = ("src", fmt, w, h, n)
    if key not in _cache:
        _cache[key] = [A.gen_clip(w, h, fmt, 0x0E0 + s, n, style=s & 1) for s in range(S)]
    return _cache[key]


def oracle(key, clip, w, h, fmt, **rate):
    if key not in _cache:
        _cache[key] = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **dict(CRF, **rate)), want_recon=True, eos=False)
    return _cache[key]


def calls_of(clips, per_call):
    return [np.ascontiguousarray(np.stack([c[k * per_call:(k + 1) * per_call] for c in clips])) for k in range(clips[0].shape[0] // per_call)]


def run(b, calls, form, pipelined=True):
    """submit / collect the calls -> streams; a held or plain device clip must come back unchanged"""
    dev = form != "host"
    junk = np.full(calls[0].size, 0xA5, dtype=np.uint8)
    ins = [b.upload(c) for c in calls] if dev else calls
    got = [b""] * b.nstreams

    def unchanged(p, c):
        back = np.zeros(c.size, dtype=np.uint8)
        b.sync()
        assert b.L.dsvg_dev_download(b.ctx, back.ctypes.data, p, back.size) == 0
        assert np.array_equal(back, c.reshape(-1)), "the caller's device clip was written (%s)" % form

    def submit(c, k):
        b.submit(c, on_device=dev, held=form == "held")
        if form == "device":                             # a plain device clip is the caller's again when submit returns
            unchanged(c, calls[k])
            assert b.L.dsvg_dev_upload(b.ctx, c, junk.ctypes.data, junk.nbytes) == 0

    def take():
        got[:] = [x + bytes(p) for x, p in zip(got, b.collect())]

    if pipelined:
        submit(ins[0], 0)
        for k, c in enumerate(ins[1:]):
            submit(c, k + 1)
            take()
        take()
    else:
        for k, c in enumerate(ins):
            submit(c, k)
            take()
    if form == "held":
        for p, c in zip(ins, calls):
            unchanged(p, c)
    return got


def fed(make, clips, form="host", pipelined=True):
    """the packets of the same session fed the numpy-composited clips, nothing set"""
    b = make()
    try:
        return run(b, calls_of(clips, F), form, pipelined)
    finally:
        b.close()


def session_list(fmt, w, h, nsrc):
    """a logo on every source for ever, a subtitle on source 0 whose fades cross the call boundary (pictures 2 .. 6 of calls of 4), and
    on the last source a slate fading in over the boundary, on top of the logo"""
    return [OV.ov(OV.bitmap(16, 9, fmt, 41), 16, 9, x=w - 22, y=4, source=-1, opacity=200),
            OV.ov(OV.bitmap(41, 11, fmt, 42), 41, 11, x=14, y=h - 14, source=0, t0=2, dur=5, fade_in=2, fade_out=2),
            OV.ov(OV.bitmap(30, 20, fmt, 43), 30, 20, x=w - 34, y=0, source=nsrc - 1, t0=3, dur=0, fade_in=3, opacity=256)]


def composited(clips, w, h, fmt, ovs, t0s=None):
    return [OV.composite(c, w, h, fmt, ovs, t0s[s] if t0s else 0, s) for s, c in enumerate(clips)]


def test_plain_batch_in_the_three_clip_forms_across_two_calls(pkg, orc):
    fmt = A.SUBSAMP_420
    clips = sources(fmt, W, H)
    ovs = session_list(fmt, W, H, S)
    assert all(OV.valid(o, W, H, fmt, S) for o in ovs)
    comp = composited(clips, W, H, fmt, ovs)
    # (the counter carries: a second call that started at picture 0 again would composite something else)
    again = OV.composite(clips[0][F:], W, H, fmt, ovs, 0, 0)
    assert not np.array_equal(again, comp[0][F:])
    want = [oracle(("b", s), comp[s], W, H, fmt, qp=80)[0] for s in range(S)]
    assert want[0] != oracle(("off", 0), clips[0], W, H, fmt, qp=80)[0]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, comp) == want
    calls = calls_of(clips, F)
    assert len(calls) == 2
    for form, pipelined in (("host", True), ("host", False), ("device", False), ("held", True)):
        b = make()
        try:
            b.set_source_overlays(pos(pkg, ovs))
            assert b.L.dsv1_batch_has_source_lane(b.h)
            got = run(b, calls, form, pipelined)
        finally:
            b.close()
        assert got == want, (form, pipelined)


def test_quality_ladder_and_chain_mode(pkg, orc):
    fmt = A.SUBSAMP_420
    qps = (60, 90)
    clips = sources(fmt, W, H)
    ovs = session_list(fmt, W, H, S)
    comp = composited(clips, W, H, fmt, ovs)
    calls = calls_of(clips, F)
    rungs = [pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=q)) for q in qps]
    want = [oracle(("l", s, q), comp[s], W, H, fmt, qp=q)[0] for s in range(S) for q in qps]
    assert fed(lambda: pkg.Ladder(rungs, S, F), comp) == want
    for form in ("host", "held"):
        b = pkg.Ladder(rungs, S, F)
        try:
            b.set_source_overlays(pos(pkg, ovs))
            got = run(b, calls, form)
        finally:
            b.close()
        assert got == want, form
    one = session_list(fmt, W, H, 1)                      # chain mode: one stream, the counter follows its pictures
    comp1 = OV.composite(clips[0], W, H, fmt, one, 0, 0)
    want = oracle(("c",), comp1, W, H, fmt, qp=75)[0]
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=75))
    for form in ("host", "device"):
        b = pkg.Batch(cfg, 1, F, chains=2)
        try:
            b.set_source_overlays(pos(pkg, one))
            got = run(b, [c[:1] for c in calls], form, pipelined=False)
        finally:
            b.close()
        assert got[0] == want, form


RF = R.rf(W, H, (6, 4, 51, 33), (96, 64), (10, 8))        # the reframe test's window of the 70 x 50 picture on its 96 x 64 canvas


def test_behind_a_uyvy_source_with_a_reframe_the_overlay_lies_in_the_bar(pkg, orc):
    fmt, sfmt, OW, OH = A.SUBSAMP_420, A.SUBSAMP_422, 96, 64
    f = PF.pf(PF.UYVY)
    planar = sources(sfmt, W, H)
    raws = [PF.pack(c.astype(np.uint32), f, W, H, sfmt, np.random.default_rng(s)).reshape(c.shape[0], -1) for s, c in enumerate(planar)]
    framed = [R.reframe_clip(CH.convert_sub(r.reshape(-1), f, W, H, sfmt, fmt, r.shape[0]), RF, fmt) for r in raws]
    # a subtitle in the bar under the window (rows 41 .. 63 are fill), a logo across the window's corner
    ovs = [OV.ov(OV.bitmap(61, 13, fmt, 51), 61, 13, x=18, y=46, source=-1, t0=1, dur=6, fade_in=1, fade_out=2),
           OV.ov(OV.bitmap(20, 12, fmt, 52), 20, 12, x=50, y=2, source=1, opacity=180)]
    assert ovs[0]["y"] >= RF["dst_y"] + RF["h"]
    comp = composited(framed, OW, OH, fmt, ovs)
    want = [oracle(("u", s), comp[s], OW, OH, fmt, qp=80)[0] for s in range(S)]
    assert want[0] != oracle(("u off", 0), framed[0], OW, OH, fmt, qp=80)[0]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(OW, OH, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, comp) == want
    rf = pkg.Reframe(RF["in_w"], RF["in_h"], (RF["x"], RF["y"], RF["w"], RF["h"]), (OW, OH), (RF["dst_x"], RF["dst_y"]), RF["fill"])
    for form, first in (("host", "overlays"), ("device", "reframe")):
        b = make()
        try:
            if first == "overlays":                       # the pass changes no geometry: any order relative to the others
                b.set_source_overlays(pos(pkg, ovs))
            b.set_source_reframe(rf)
            b.set_source_format(pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"]), src_subsamp=sfmt)
            if first == "reframe":
                b.set_source_overlays(pos(pkg, ovs))
            got = run(b, calls_of(raws, F), form)
        finally:
            b.close()
        assert got == want, form


def test_overlay_seek(pkg, orc):
    fmt = A.SUBSAMP_420
    clips = sources(fmt, W, H)
    ovs = session_list(fmt, W, H, S)
    # source 0 plays pictures 1 .. 4 and then, after a seek, 2 .. 5 again; source 1 pictures 0 .. 3 and then 100 ..
    first = [OV.composite(clips[0][:F], W, H, fmt, ovs, 1, 0), OV.composite(clips[1][:F], W, H, fmt, ovs, 0, 1)]
    second = [OV.composite(clips[0][F:], W, H, fmt, ovs, 2, 0), OV.composite(clips[1][F:], W, H, fmt, ovs, 100, 1)]
    comp = [np.concatenate([first[s], second[s]]) for s in range(S)]
    want = [oracle(("seek", s), comp[s], W, H, fmt, qp=80)[0] for s in range(S)]
    calls = calls_of(clips, F)
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    try:
        b.set_source_overlays(pos(pkg, ovs))
        b.overlay_seek(-1, 7)
        b.overlay_seek(0, 1)
        b.overlay_seek(1, 0)
        p1 = b.encode(calls[0])
        b.overlay_seek(0, 2)
        b.overlay_seek(1, 100)
        p2 = b.encode(calls[1])
        assert b.L.dsv1_batch_overlay_seek(b.h, 2, 0) == DSVG_ERR_ARG and b.L.dsv1_batch_overlay_seek(b.h, -2, 0) == DSVG_ERR_ARG
    finally:
        b.close()
    assert [bytes(x) + bytes(y) for x, y in zip(p1, p2)] == want


LW, LH = 128, 96


def ladder_run(b, calls, form):
    dev = form != "host"
    ins = [b.upload(c) for c in calls] if dev else calls
    got, xs, xp = [b""] * b.nstreams, [], []
    for c in ins:
        b.submit(c, on_device=dev, held=form == "held")
    for _ in ins:
        got[:] = [x + bytes(p) for x, p in zip(got, b.collect())]
        xs.append(b.src_sse())
        xp.append(b.src_psnr())
    return got, np.concatenate(xs, axis=1), np.concatenate(xp, axis=1)


def test_resolution_ladder(pkg, orc):
    fmt = A.SUBSAMP_420
    shapes = [(LW, LH, 80), (LW // 2, LH // 2, 70)]      # one geometry of the source's own size
    clips = sources(fmt, LW, LH)
    ovs = session_list(fmt, LW, LH, S)
    comp = composited(clips, LW, LH, fmt, ovs)
    want = []
    for s, clip in enumerate(comp):
        for gw, gh, qp in shapes:
            sc = clip if (gw, gh) == (LW, LH) else Z.scale_clip(clip, LW, LH, fmt, gw, gh, Z.CUBIC)
            want.append(oracle(("r", s, gw), sc, gw, gh, fmt, qp=qp)[0])
    geoms = lambda: [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, qp=qp))]) for gw, gh, qp in shapes]
    # the ladder fed the composited clip: packets and source-resolution figures to compare with
    b = pkg.ResLadder(LW, LH, fmt, geoms(), S, F, Z.CUBIC)
    try:
        b.src_quality_enable(sse=True, ssim=False, filt=Z.CUBIC)
        base, bsse, bpsnr = ladder_run(b, calls_of(comp, F), "host")
    finally:
        b.close()
    assert base == want
    # (measured against the clips as they came in, the figures would differ)
    b = pkg.ResLadder(LW, LH, fmt, geoms(), S, F, Z.CUBIC)
    try:
        b.src_quality_enable(sse=True, ssim=False, filt=Z.CUBIC)
        _, osse, _ = ladder_run(b, calls_of(clips, F), "host")
    finally:
        b.close()
    assert not np.array_equal(osse, bsse)
    for form in ("host", "device", "held"):
        b = pkg.ResLadder(LW, LH, fmt, geoms(), S, F, Z.CUBIC)
        try:
            b.set_overlays(pos(pkg, ovs))
            b.src_quality_enable(sse=True, ssim=False, filt=Z.CUBIC)
            got, xsse, xpsnr = ladder_run(b, calls_of(clips, F), form)
        finally:
            b.close()
        assert got == want, form
        assert np.array_equal(xsse, bsse) and np.array_equal(xpsnr, bpsnr), form            # src_psnr() is against the OVERLAID source
    # seek: the second call shows the first call's clip at the first call's pictures again
    b = pkg.ResLadder(LW, LH, fmt, geoms(), S, F, Z.CUBIC)
    ref = pkg.ResLadder(LW, LH, fmt, geoms(), S, F, Z.CUBIC)
    try:
        b.set_overlays(pos(pkg, ovs))
        call, ccall = calls_of(clips, F)[0], calls_of(comp, F)[0]
        assert [bytes(x) for x in b.encode(call)] == [bytes(x) for x in ref.encode(ccall)]
        b.overlay_seek(-1, 0)
        assert [bytes(x) for x in b.encode(call)] == [bytes(x) for x in ref.encode(ccall)]
        assert b.L.dsv1_resladder_overlay_seek(b.h, S, 0) == DSVG_ERR_ARG
    finally:
        b.close()
        ref.close()


# ---- errors and the feature off --------------------------------------------------------------------------------------------------
def test_error_contract(pkg, orc):
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    clips = sources(fmt, W, H)[:1]
    ovs = session_list(fmt, W, H, 1)
    comp = OV.composite(clips[0], W, H, fmt, ovs, 0, 0)
    want = oracle(("e",), comp, W, H, fmt, qp=80)[0]
    plain = oracle(("off", 0), clips[0], W, H, fmt, qp=80)[0]
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80))
    calls = calls_of(clips, F)
    setter = L.dsv1_batch_set_source_overlays
    good = pkg._overlay_array(pos(pkg, ovs))[0]
    bads = []
    for change in (dict(x=W - 10), dict(x=15), dict(y=5), dict(opacity=257), dict(source=1), dict(reserved=1), dict(w=0), dict(planes=None)):
        bads.append(pkg._overlay_array(pos(pkg, [ovs[0], dict(ovs[1], **change), ovs[2]]))[0])
    b = pkg.Batch(cfg, 1, F)
    try:
        # no list: seek is refused; NULL, 0 and an empty list clear the pass: no lane
        assert L.dsv1_batch_overlay_seek(b.h, -1, 0) == DSVG_ERR_ARG
        b.set_source_overlays(pos(pkg, ovs))
        assert L.dsv1_batch_has_source_lane(b.h)
        b.set_source_overlays(None)
        assert not L.dsv1_batch_has_source_lane(b.h)
        assert L.dsv1_batch_overlay_seek(b.h, -1, 0) == DSVG_ERR_ARG
        b.set_source_overlays(pos(pkg, ovs))
        assert setter(b.h, good, 0) == 0 and not L.dsv1_batch_has_source_lane(b.h)
        b.set_source_overlays([])
        assert not L.dsv1_batch_has_source_lane(b.h)
        assert setter(b.h, good, -1) == DSVG_ERR_ARG and setter(b.h, good, OV.MAX_OVERLAYS + 1) == DSVG_ERR_ARG
        assert setter(None, good, 3) == DSVG_ERR_ARG
        # a clip staged, a batch in flight: refused, and the batch codes the clips themselves
        pin = b.pinned(calls[0].shape)
        pin[...] = calls[0]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == 0
        assert setter(b.h, good, 3) == DSVG_ERR_ARG
        b.submit(pin)
        assert setter(b.h, good, 3) == DSVG_ERR_ARG and setter(b.h, None, 0) == DSVG_ERR_ARG
        p1 = bytes(b.collect()[0])
        assert not L.dsv1_batch_has_source_lane(b.h)
        assert p1 + bytes(b.encode(calls[1])[0]) == plain
    finally:
        b.close()
    b = pkg.Batch(cfg, 1, F)
    try:
        b.set_source_overlays(pos(pkg, ovs))
        pin = b.pinned(calls[0].shape)
        pin[...] = calls[0]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == DSVG_ERR_ARG                                          # stage is refused while set
        for bad in bads:                                                                                         # an invalid item: as it was
            assert setter(b.h, bad, 3) == DSVG_ERR_ARG
        b.submit(pin)
        assert setter(b.h, good, 3) == DSVG_ERR_ARG and setter(b.h, None, 0) == DSVG_ERR_ARG                       # in flight: as it was
        first = b.collect()[0]
        assert bytes(first) + bytes(b.encode(calls[1])[0]) == want
        # the other passes come and go around it
        assert L.dsv1_batch_set_source_orient(b.h, 1) == 0 and L.dsv1_batch_set_source_orient(b.h, 0) == 0
        assert L.dsv1_batch_has_source_lane(b.h)
        b.set_source_overlays(None)
        assert not L.dsv1_batch_has_source_lane(b.h)
    finally:
        b.close()
    # the resolution ladder's setters
    r = pkg.ResLadder(LW, LH, fmt, [(LW, LH, [pkg.make_encoder_cfg(LW, LH, fmt, **dict(CRF, qp=80))])], 1, F, Z.CUBIC)
    try:
        lovs = pkg._overlay_array(pos(pkg, session_list(fmt, LW, LH, 1)))[0]
        assert L.dsv1_resladder_set_overlays(None, lovs, 3) == DSVG_ERR_ARG
        assert L.dsv1_resladder_overlay_seek(r.h, -1, 0) == DSVG_ERR_ARG
        assert L.dsv1_resladder_set_overlays(r.h, bads[1], 3) == DSVG_ERR_ARG             # (x = 15: not aligned on any canvas)
        assert L.dsv1_resladder_set_overlays(r.h, lovs, 3) == 0
        r.overlay_seek(0, 5)
        r.submit(calls_of(sources(fmt, LW, LH)[:1], F)[0])
        assert L.dsv1_resladder_set_overlays(r.h, lovs, 3) == DSVG_ERR_ARG and L.dsv1_resladder_set_overlays(r.h, None, 0) == DSVG_ERR_ARG
        r.collect()
        r.set_overlays(None)
        assert L.dsv1_resladder_overlay_seek(r.h, -1, 0) == DSVG_ERR_ARG
    finally:
        r.close()
    # the standalone call
    src = noise(1, W, H, fmt, 2)
    keep = src.copy()
    assert L.dsv1_overlay_clip(0, None, W, H, fmt, 1, good, 3, 0, 0) == DSVG_ERR_ARG
    assert L.dsv1_overlay_clip(0, src.ctypes.data, W, H, fmt, 0, good, 3, 0, 0) == DSVG_ERR_ARG
    assert L.dsv1_overlay_clip(0, src.ctypes.data, W, H, fmt, 1, None, 3, 0, 0) == DSVG_ERR_ARG
    assert L.dsv1_overlay_clip(0, src.ctypes.data, W, H, 0x7, 1, good, 3, 0, 0) == DSVG_ERR_ARG
    for bad in bads:
        assert L.dsv1_overlay_clip(0, src.ctypes.data, W, H, fmt, 1, bad, 3, 0, 0) == DSVG_ERR_ARG
    assert np.array_equal(src, keep)


def test_feature_off(pkg, orc):
    """a batch that never calls the setter, one that set and cleared a list, and one whose list is never active in its calls write the
    oracle's streams of the clip itself; the first two hold no lane"""
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    clips = sources(fmt, W, H)
    want = [oracle(("off", s), clips[s], W, H, fmt, qp=80)[0] for s in range(S)]
    calls = calls_of(clips, F)
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80))
    ovs = session_list(fmt, W, H, S)
    late = [dict(o, t0=1000, dur=10) for o in ovs] + [dict(ovs[0], opacity=0)]
    assert OV.plan(late, S, F, [0, 0]) == ([], 0) and OV.plan(late, S, F, [F, F]) == ([], 0)
    for mode in ("never", "cleared", "empty"):
        b = pkg.Batch(cfg, S, F)
        try:
            if mode != "never":
                b.set_source_overlays(pos(pkg, ovs))
                assert L.dsv1_batch_has_source_lane(b.h)
                b.set_source_overlays(None if mode == "cleared" else [])
            assert not L.dsv1_batch_has_source_lane(b.h), mode
            pin = b.pinned(calls[0].shape)
            pin[...] = calls[0]
            assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == 0, mode                                            # nothing set: stage works
            b.submit(pin)
            first = b.collect()
            got = [bytes(x) + bytes(y) for x, y in zip(first, b.encode(calls[1]))]
        finally:
            b.close()
        assert got == want, mode
    for form, pipelined in (("host", True), ("device", False), ("held", True)):
        b = pkg.Batch(cfg, S, F)
        try:
            b.set_source_overlays(pos(pkg, late))
            got = run(b, calls, form, pipelined)
        finally:
            b.close()
        assert got == want, ("never active", form)
    # ... and the counter went on counting through those calls: a list that wakes up in the third call's pictures
    wake = [dict(ovs[0], t0=2 * F + 1, dur=2, source=-1)]
    third = composited([c[:F] for c in clips], W, H, fmt, wake, [2 * F, 2 * F])
    assert not np.array_equal(third[0], clips[0][:F])
    b = pkg.Batch(cfg, S, F)
    fedb = pkg.Batch(cfg, S, F)
    try:
        b.set_source_overlays(pos(pkg, wake))
        for c, d in ((calls[0], calls[0]), (calls[1], calls[1]), (calls[0], calls_of(third, F)[0])):
            got, ref = b.encode(c), fedb.encode(d)
            assert [bytes(x) for x in got] == [bytes(x) for x in ref]
    finally:
        b.close()
        fedb.close()
