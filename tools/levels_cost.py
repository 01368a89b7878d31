#!/usr/bin/env python3
"""What the levels pass and the histogram cost (dsv1_levels_clip, dsv1_histogram_clip, dsv1_batch_set_source_levels;
csrc/k_levels.hip), 1920x1080 4:2:0, on one MI355X.

profiles/levels_cost.txt is kept in sections, each opened by a line "== name: title"; this tool rewrites the sections it measures and
leaves every other section as it finds it:

    python tools/levels_cost.py [--frames 96] [--rounds 9] [--reps 10]
        section "levels": k_levels with its table replicated 32 times in LDS (the pass as sessions run it) and with one copy
        (dsvg_levels_set_replicas), on a noise clip and on a flat clip resident in HBM, in place and out of place; the plain kernel of
        tools/ubench/levels_naive.hip on the same clip; a hipMemcpyAsync device-to-device of the same bytes on the same stream -- all
        alternating, each timed with device events around `--reps` back-to-back enqueues, round 0 thrown away as the warm-up.
        section "histogram": k_histogram on the noise clip and on the flat clip, per picture and as bytes per second of the bytes
        read, and the plain kernel on the first `--naive-frames` pictures of each (one global atomic per sample: a flat picture
        serialises on three addresses, so it gets few pictures).
    The results of the three levels kernels, and of the two histograms, are compared before anything is timed.

The plain kernels are built from tools/ubench/levels_naive.hip into tools/ubench/liblevels_naive.so where that is missing (--naive names
another file).  Compulsory bytes: levels one byte read and one written per sample, the histogram one byte read.  The ratios are
measurements of this code against a copy and against the plain kernels on one box in one run, not targets."""
import argparse
import ctypes as C
import datetime
import os
import statistics
import subprocess
import sys

HERE = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
W, H = 1920, 1080
FB = W * H * 3 // 2                                       # 4:2:0
HEAD = "Cost of the levels pass and the histogram (csrc/k_levels.hip); written by tools/levels_cost.py, section by section"


def setup(root):
    import importlib
    sys.path.insert(0, os.path.join(root, "tests"))
    sys.path.insert(0, root)
    import _cabi as A
    assert A.frame_bytes(W, H, A.SUBSAMP_420) == FB
    return importlib.import_module("digital-subband-video-1_amd"), A


def naive_lib(path):
    src = os.path.join(HERE, "tools", "ubench", "levels_naive.hip")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-o", path, src], check=True)
    L = C.CDLL(path)
    L.levels_naive.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.histogram_naive.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    return L


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
    return "median %.3f ms, min %.3f ms, max %.3f ms (spread %.2f %% of the median)" % (med * scale, min(ts) * scale, max(ts) * scale, 100 * (max(ts) - min(ts)) / med)


def measure(root, n, rounds, reps, nn, naive_path):
    import numpy as np
    pkg, A = setup(root)
    import _levels as LV
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    hip = Hip()
    NL = naive_lib(naive_path)
    L.dsvg_lane_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.dsvg_lane_stream.argtypes = [C.c_void_p]
    L.dsvg_lane_stream.restype = C.c_void_p
    L.dsvg_lane_sync.argtypes = [C.c_void_p]
    L.dsvg_lane_destroy.argtypes = [C.c_void_p]
    L.dsvg_levels_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(pkg.Levels), C.c_int, C.c_int, C.c_int]
    L.dsvg_levels_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.dsvg_levels_set_replicas.argtypes = [C.c_void_p, C.c_int]
    L.dsvg_levels_destroy.argtypes = [C.c_void_p]
    L.dsvg_histogram_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]
    L.dsvg_histogram_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.dsvg_histogram_destroy.argtypes = [C.c_void_p]
    nn = min(nn, n)
    mem = pkg.Batch(pkg.make_encoder_cfg(64, 64, fmt), 1, 1)
    lane, lv32, lv1, hg = C.c_void_p(None), C.c_void_p(None), C.c_void_p(None), C.c_void_p(None)
    try:
        def dev(nbytes):
            p = C.c_void_p(None)
            assert L.dsvg_dev_alloc(mem.ctx, C.byref(p), nbytes) == 0
            return p

        def host(p, nbytes, dtype=np.uint8):
            out = np.zeros(nbytes, dtype=np.uint8)
            assert L.dsvg_dev_download(mem.ctx, out.ctypes.data, p, nbytes) == 0
            return out.view(dtype)

        tables = LV.compose(LV.range_(1, 0), LV.adjust(24, 228, 16, 235, 300))
        noise_h = np.random.default_rng(0xD0).integers(0, 256, size=(12, FB), dtype=np.uint8)
        noise = mem.upload(np.ascontiguousarray(np.tile(noise_h, (n // 12 + 1, 1))[:n]))
        flat = mem.upload(np.full((n, FB), 128, dtype=np.uint8))
        lut = mem.upload(np.ascontiguousarray(tables))
        out, plain, other, work = dev(n * FB), dev(n * FB), dev(n * FB), dev(n * FB)
        hist, hist_n = dev(n * 768 * 4), dev(n * 768 * 4)
        assert L.dsvg_lane_create(C.byref(lane), 0) == 0
        st = L.dsvg_lane_stream(lane)
        t_ = pkg.Levels.from_tables(tables)
        assert L.dsvg_levels_create(C.byref(lv32), 0, C.byref(t_), W, H, fmt) == 0
        assert L.dsvg_levels_create(C.byref(lv1), 0, C.byref(t_), W, H, fmt) == 0 and L.dsvg_levels_set_replicas(lv1, 1) == 0
        assert L.dsvg_histogram_create(C.byref(hg), 0, W, H, fmt) == 0

        def levels(p, src, dst):
            def fn():
                assert L.dsvg_levels_run(p, st, src, n, dst) == 0
            return fn

        def naive_levels():
            assert NL.levels_naive(st, noise, plain, lut, W, H, 1, 1, n) == 0

        def copy():
            hip.d2d(other, noise, n * FB, st)

        def histogram(src, k=n):
            def fn():
                assert L.dsvg_histogram_run(hg, st, src, k, hist) == 0
            return fn

        def naive_histogram(src):
            def fn():
                assert NL.histogram_naive(st, src, hist_n, W, H, 1, 1, nn) == 0
            return fn

        # the three levels kernels write the same frames; the two histograms count the same
        want = LV.levels_clip(noise_h[:2], W, H, fmt, tables).reshape(-1)
        for name, fn, where in (("32 copies", levels(lv32, noise, out), out), ("1 copy", levels(lv1, noise, out), out), ("plain", naive_levels, plain)):
            fn()
            assert L.dsvg_lane_sync(lane) == 0
            assert np.array_equal(host(where, 2 * FB), want), "k_levels (%s) and the numpy statement disagree" % name
        hip.d2d(work, noise, n * FB, st)
        levels(lv32, work, work)()
        assert L.dsvg_lane_sync(lane) == 0
        assert np.array_equal(host(work, 2 * FB), want), "k_levels in place and the numpy statement disagree"
        for name, src, ref in (("noise", noise, LV.histogram(noise_h[:nn], W, H, fmt) if nn <= 12 else None), ("flat", flat, None)):
            histogram(src, nn)()
            naive_histogram(src)()
            assert L.dsvg_lane_sync(lane) == 0
            a, b = host(hist, nn * 768 * 4, np.uint32), host(hist_n, nn * 768 * 4, np.uint32)
            assert np.array_equal(a, b), "k_histogram and the plain kernel disagree (%s)" % name
            assert ref is None or np.array_equal(a.reshape(ref.shape), ref), "k_histogram and np.bincount disagree"
        fns = (("rep32 noise", levels(lv32, noise, out), reps), ("rep1 noise", levels(lv1, noise, out), reps), ("rep32 flat", levels(lv32, flat, out), reps),
               ("rep1 flat", levels(lv1, flat, out), reps), ("rep32 in place", levels(lv32, work, work), reps), ("naive", naive_levels, reps), ("copy", copy, reps),
               ("hist noise", histogram(noise), reps), ("hist flat", histogram(flat), reps),
               ("naive hist noise", naive_histogram(noise), 1), ("naive hist flat", naive_histogram(flat), 1))
        t = {name: [] for name, _, _ in fns}
        for r in range(rounds + 1):
            for name, fn, k in fns:
                if name.startswith("naive hist") and r > 3:
                    continue                             # (three timed rounds of the slow ones)
                s = hip.timed(st, fn, k)
                if r:                                    # (round 0 warms up)
                    t[name].append(s)
        assert L.dsvg_lane_sync(lane) == 0
    finally:
        if lane:
            L.dsvg_lane_sync(lane)
        for p in (lv32, lv1):
            if p:
                L.dsvg_levels_destroy(p)
        if hg:
            L.dsvg_histogram_destroy(hg)
        if lane:
            L.dsvg_lane_destroy(lane)
        mem.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    today = datetime.date.today().isoformat()
    tbs = lambda s: 2 * n * FB / s / 1e12
    lv = ["%dx%d 4:2:0, %d pictures resident in HBM; device events around %d back-to-back enqueues on one stream, %d timed rounds after one" % (W, H, n, reps, rounds),
          "warm-up round, all alternating.  Every one of them reads %d bytes and writes %d per call.  Tables: full -> limited range composed" % (n * FB, n * FB),
          "with a black / white point and saturation adjustment.  Measured %s." % today]
    names = (("rep32 noise", "k_levels, 32 copies, noise:  "), ("rep1 noise", "k_levels, 1 copy, noise:    "), ("rep32 flat", "k_levels, 32 copies, flat:   "),
             ("rep1 flat", "k_levels, 1 copy, flat:     "), ("rep32 in place", "k_levels, 32 copies, in place:"), ("naive", "plain kernel, noise:        "),
             ("copy", "hipMemcpyAsync D2D:         "))
    lv += ["%s %s; %.2f TB/s read + written" % (title, stats(t[k]), tbs(med[k])) for k, title in names]
    lv += ["ratios (time): 32 copies / copy %.2f (noise) %.2f (flat), 1 copy / copy %.2f (noise) %.2f (flat), in place / copy %.2f, 32 copies / plain kernel %.2f (plain kernel / copy %.2f)" % (
               med["rep32 noise"] / med["copy"], med["rep32 flat"] / med["copy"], med["rep1 noise"] / med["copy"], med["rep1 flat"] / med["copy"],
               med["rep32 in place"] / med["copy"], med["rep32 noise"] / med["naive"], med["naive"] / med["copy"]),
           "per picture: 32 copies %.2f us, 1 copy %.2f us, plain kernel %.2f us, copy %.2f us (noise)" % tuple(med[k] * 1e6 / n for k in ("rep32 noise", "rep1 noise", "naive", "copy"))]
    hs = ["The same clips and method.  k_histogram reads %d bytes per call (%d pictures); the plain kernel (one global atomic per sample) is timed on" % (n * FB, n),
          "the first %d pictures, one enqueue per timing, three timed rounds.  Measured %s." % (nn, today)]
    for k, title, cnt in (("hist noise", "k_histogram, noise: ", n), ("hist flat", "k_histogram, flat:  ", n), ("naive hist noise", "plain kernel, noise:", nn),
                          ("naive hist flat", "plain kernel, flat: ", nn)):
        hs.append("%s %s; %.2f us per picture, %.3f TB/s read" % (title, stats(t[k]), med[k] * 1e6 / cnt, cnt * FB / med[k] / 1e12))
    hs.append("ratios (time per picture): flat / noise %.2f (k_histogram), k_histogram / plain kernel %.4f (noise) %.5f (flat)" % (
        med["hist flat"] / med["hist noise"], (med["hist noise"] / n) / (med["naive hist noise"] / nn), (med["hist flat"] / n) / (med["naive hist flat"] / nn)))
    return lv, hs


def read_sections(path):
    secs = []
    if os.path.exists(path):
        for line in open(path).read().splitlines():
            if line.startswith("== "):
                name, _, title = line[3:].partition(":")
                secs.append((name.strip(), title.strip(), []))
            elif secs:
                secs[-1][2].append(line)
    return secs


def write_section(path, sec):
    secs = read_sections(path)
    secs = [sec if s[0] == sec[0] else s for s in secs] if sec[0] in [s[0] for s in secs] else secs + [sec]
    with open(path, "w") as f:
        f.write(HEAD + "\n")
        for name, title, lines in secs:
            while lines and not lines[-1].strip():
                lines = lines[:-1]
            f.write("\n== %s: %s\n%s\n" % (name, title, "\n".join(lines)))
    print("== %s\n%s" % (sec[0], "\n".join(sec[2])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--naive-frames", type=int, default=2, help="pictures the plain histogram kernel is timed on")
    ap.add_argument("--root", default=HERE, help="the built tree of the project to measure (default: this one)")
    ap.add_argument("--naive", default=os.path.join(HERE, "tools", "ubench", "liblevels_naive.so"), help="the plain kernels' shared library")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "levels_cost.txt"))
    a = ap.parse_args()
    lv, hs = measure(os.path.abspath(a.root), a.frames, a.rounds, a.reps, a.naive_frames, a.naive)
    write_section(a.out, ("levels", "k_levels against a device-to-device copy and a plain kernel (python tools/levels_cost.py)", lv))
    write_section(a.out, ("histogram", "k_histogram on a noise clip and on a flat clip, against a plain kernel (python tools/levels_cost.py)", hs))


if __name__ == "__main__":
    main()
