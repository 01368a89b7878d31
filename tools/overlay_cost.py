#!/usr/bin/env python3
"""What the overlay pass costs (dsv1_overlay_clip, dsv1_batch_set_source_overlays; csrc/k_overlay.hip), 1920x1080 4:2:0, 96 pictures, on
one MI355X.

    python tools/overlay_cost.py [--frames 96] [--rounds 9] [--reps 10]

Three lists of one overlay each, visible on every picture at op 256 with a random alpha plane: a 200x80 logo, a 1920x120 subtitle
band, a full-frame slate.  For each:
  * the pass on a clip resident in HBM -- dsvg_overlay_run: the plan, the table's upload and one launch, in place -- timed with device
    events around `--reps` back-to-back enqueues on one stream, alternating with a hipMemcpyAsync device-to-device copy of the WHOLE
    clip on the same stream (what a pass that worked out of place would pay at least), round 0 thrown away as the warm-up;
  * dsv1_overlay_clip on the same clip in pinned host memory, wall clock: the round trip over the link a caller pays who composites on
    the GPU but keeps the clip on the host -- and less than what a caller pays today, who composites on the host as well.
The result of the pass is compared with tests/_overlay.py on the first two pictures before anything is timed.
Then the one structural claim: the logo's cost on 96 pictures of 1280x720, 1920x1080 and 3840x2160 -- the work is the overlay's area,
not the picture's.  profiles/overlay_cost.txt holds what this printed; the figures are measurements of this code on one box in one run,
not targets."""
import argparse
import ctypes as C
import datetime
import os
import statistics
import sys
import time

HERE = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
W, H = 1920, 1080
CASES = (("logo 200x80", 200, 80, 1680, 40), ("subtitle band 1920x120", 1920, 120, 0, 920), ("full-frame slate 1920x1080", 1920, 1080, 0, 0))


def setup(root):
    import importlib
    sys.path.insert(0, os.path.join(root, "tests"))
    sys.path.insert(0, root)
    import _cabi as A
    import _overlay as OV
    return importlib.import_module("digital-subband-video-1_amd"), A, OV


class Hip:
    """the few runtime calls the timing needs, from the runtime the library is linked against"""

    def __init__(self):
        self.L = C.CDLL("libamdhip64.so")
        self.L.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.L.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.L.hipEventSynchronize.argtypes = [C.c_void_p]
        self.L.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.a, self.b = C.c_void_p(None), C.c_void_p(None)
        assert self.L.hipEventCreate(C.byref(self.a)) == 0 and self.L.hipEventCreate(C.byref(self.b)) == 0

    def timed(self, stream, fn, reps):
        """seconds per repetition of fn, `reps` enqueues between two events on the stream"""
        ms = C.c_float(0)
        assert self.L.hipEventRecord(self.a, stream) == 0
        for _ in range(reps):
            fn()
        assert self.L.hipEventRecord(self.b, stream) == 0 and self.L.hipEventSynchronize(self.b) == 0
        assert self.L.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value * 1e-3 / reps

    def d2d(self, dst, src, nbytes, stream):
        assert self.L.hipMemcpyAsync(dst, src, nbytes, 3, stream) == 0          # hipMemcpyDeviceToDevice


def stats(ts, scale=1e3):
    med = statistics.median(ts)
    return "median %.3f ms, min %.3f ms, max %.3f ms" % (med * scale, min(ts) * scale, max(ts) * scale)


def measure(root, n, rounds, reps):
    import numpy as np
    pkg, A, OV = setup(root)
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    hip = Hip()
    L.dsvg_lane_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.dsvg_lane_stream.argtypes = [C.c_void_p]
    L.dsvg_lane_stream.restype = C.c_void_p
    L.dsvg_lane_sync.argtypes = [C.c_void_p]
    L.dsvg_lane_destroy.argtypes = [C.c_void_p]
    L.dsvg_overlay_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(pkg.Overlay), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.dsvg_overlay_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.dsvg_overlay_destroy.argtypes = [C.c_void_p]
    mem = pkg.Batch(pkg.make_encoder_cfg(64, 64, fmt), 1, 1)
    lane = C.c_void_p(None)
    passes = []
    zero = C.c_int64(0)
    out = []
    try:
        assert L.dsvg_lane_create(C.byref(lane), 0) == 0
        st = L.dsvg_lane_stream(lane)

        def dev(nbytes):
            p = C.c_void_p(None)
            assert L.dsvg_dev_alloc(mem.ctx, C.byref(p), nbytes) == 0
            return p

        def clip_of(w, h):
            fb = A.frame_bytes(w, h, fmt)
            base = np.random.default_rng(0xC0 + w).integers(0, 256, size=(4, fb), dtype=np.uint8)
            return fb, base, mem.upload(np.ascontiguousarray(np.tile(base, (n // 4 + 1, 1))[:n]))

        def make(w, h, ow, oh, x, y, seed):
            o = OV.ov(OV.bitmap(ow, oh, fmt, seed), ow, oh, x=x, y=y)
            arr, cnt = pkg._overlay_array([pkg.Overlay(o["planes"], ow, oh, x, y)])
            p = C.c_void_p(None)
            assert L.dsvg_overlay_create(C.byref(p), 0, arr, cnt, w, h, fmt, 1) == 0
            passes.append(p)
            return o, p

        def run(p, clip):
            def fn():
                assert L.dsvg_overlay_run(p, st, 0, clip, n, C.byref(zero)) == 0
            return fn

        def check(o, p, w, h, fb, base, clip, work):
            hip.d2d(work, clip, n * fb, st)
            run(p, work)()
            assert L.dsvg_lane_sync(lane) == 0
            got = np.zeros(2 * fb, dtype=np.uint8)
            assert L.dsvg_dev_download(mem.ctx, got.ctypes.data, work, got.size) == 0
            assert np.array_equal(got.reshape(2, fb), OV.composite(base[:2], w, h, fmt, [o], 0)), "k_overlay and the numpy statement disagree"

        fb, base, clip = clip_of(W, H)
        work, other = dev(n * fb), dev(n * fb)
        pin = mem.pinned((n, fb))
        pin[...] = np.tile(base, (n // 4 + 1, 1))[:n]
        fns, hosts = [], []
        for k, (name, ow, oh, x, y) in enumerate(CASES):
            o, p = make(W, H, ow, oh, x, y, 7 + k)
            check(o, p, W, H, fb, base, clip, work)
            fns.append((name, run(p, work)))
            lst = [pkg.Overlay(o["planes"], ow, oh, x, y)]
            hosts.append((name, lambda lst=lst: L.dsv1_overlay_clip(0, pin.ctypes.data, W, H, fmt, n, pkg._overlay_array(lst)[0], 1, 0, 0)))
        fns.append(("copy", lambda: hip.d2d(other, clip, n * fb, st)))
        t = {name: [] for name, _ in fns}
        for r in range(rounds + 1):
            for name, fn in fns:
                s = hip.timed(st, fn, reps)
                if r:                                    # (round 0 warms up)
                    t[name].append(s)
        assert L.dsvg_lane_sync(lane) == 0
        th = {name: [] for name, _ in hosts}
        for r in range(4):
            for name, fn in hosts:
                t0 = time.perf_counter()
                assert fn() == 0
                if r:
                    th[name].append(time.perf_counter() - t0)
        med = {k: statistics.median(v) for k, v in t.items()}
        today = datetime.date.today().isoformat()
        out += ["%dx%d 4:2:0, %d pictures (%d bytes) resident in HBM; device events around %d back-to-back enqueues on one stream, %d timed rounds" % (W, H, n, n * fb, reps, rounds),
                "after one warm-up round, all alternating.  One overlay, every picture, op 256, random alpha; in place.  A call is the plan on the",
                "host, the table's upload and one launch.  Measured %s." % today,
                "hipMemcpyAsync D2D of the clip:   %s; %.2f us per picture" % (stats(t["copy"]), med["copy"] * 1e6 / n)]
        for name, ow, oh, _, _ in CASES:
            area = ow * oh * 3 // 2
            out.append("%-33s %s; %.2f us per picture; %.3f of the copy's time; %.2f TB/s of the %d bytes a picture's blend reads and writes" % (
                name + ":", stats(t[name]), med[name] * 1e6 / n, med[name] / med["copy"], 4 * area * n / med[name] / 1e12, 4 * area))
        out.append("dsv1_overlay_clip on the same clip in pinned host memory (upload, the pass, download, one lane and one list per call), wall clock, 3 timed calls:")
        for name, _, _, _, _ in CASES:
            m = statistics.median(th[name])
            out.append("%-33s median %.1f ms; %.0f times the resident pass" % (name + ":", m * 1e3, m / med[name]))
        # the logo on three picture sizes
        out.append("The 200x80 logo, %d pictures, by picture size (the same method):" % n)
        logo = {}
        sizes = ((1280, 720), (1920, 1080), (3840, 2160))
        clips = []
        for w, h in sizes:
            fb2, base2, clip2 = clip_of(w, h)
            work2 = dev(n * fb2)
            o, p = make(w, h, 200, 80, w - 240, 40, 99)
            check(o, p, w, h, fb2, base2, clip2, work2)
            clips.append((w, h, run(p, work2)))
        ts = {(w, h): [] for w, h, _ in clips}
        for r in range(rounds + 1):
            for w, h, fn in clips:
                s = hip.timed(st, fn, reps)
                if r:
                    ts[(w, h)].append(s)
        for w, h in sizes:
            m = statistics.median(ts[(w, h)])
            logo[(w, h)] = m
            out.append("  %4dx%-4d %s; %.2f us per picture" % (w, h, stats(ts[(w, h)]), m * 1e6 / n))
        out.append("  3840x2160 / 1280x720: %.2f in time, %.2f in picture bytes" % (logo[sizes[2]] / logo[sizes[0]], 9.0))
    finally:
        if lane:
            L.dsvg_lane_sync(lane)
        for p in passes:
            L.dsvg_overlay_destroy(p)
        if lane:
            L.dsvg_lane_destroy(lane)
        mem.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--root", default=HERE, help="the built tree of the project to measure (default: this one)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "overlay_cost.txt"))
    a = ap.parse_args()
    lines = measure(os.path.abspath(a.root), a.frames, a.rounds, a.reps)
    text = "Cost of the overlay pass (csrc/k_overlay.hip); written by tools/overlay_cost.py\n\n" + "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
