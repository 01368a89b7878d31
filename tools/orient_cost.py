#!/usr/bin/env python3
"""What the orientation pass costs (dsv1_orient_clip, dsv1_batch_set_source_orient; csrc/k_orient.hip), 1920x1080 4:2:0, on one
MI355X.

profiles/orient_cost.txt is kept in sections, each opened by a line "== name: title"; this tool rewrites the section it measures and
leaves every other section as it finds it:

    python tools/orient_cost.py [--frames 96] [--rounds 9] [--reps 10]
        section "orient": k_orient_rows (HFLIP, ROT180) and k_orient_tr (ROT90) on a device-resident clip of a batch's size, the plain
        ROT90 kernel of tools/ubench/orient_naive.hip on the same clip, and a hipMemcpyAsync device-to-device of the same OUTPUT bytes
        on the same stream -- the five alternating, each timed with device events around `--reps` back-to-back enqueues, round 0
        thrown away as the warm-up.  The plain kernel's frames are compared with the pass's before anything is timed.

The plain kernel is built from tools/ubench/orient_naive.hip into tools/ubench/liborient_naive.so where that is missing (--naive names
another file).  Compulsory bytes of the pass: one byte read and one byte written per sample.  The ratios are measurements of this code
against a copy and against the plain kernel on one box in one run, not targets."""
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
HFLIP, ROT180, ROT90 = 1, 3, 5
HEAD = "Cost of the orientation pass (csrc/k_orient.hip); written by tools/orient_cost.py, section by section"


def setup(root):
    import importlib
    sys.path.insert(0, os.path.join(root, "tests"))
    sys.path.insert(0, root)
    import _cabi as A
    assert A.frame_bytes(W, H, A.SUBSAMP_420) == FB
    return importlib.import_module("digital-subband-video-1_amd"), A


def naive_lib(path):
    src = os.path.join(HERE, "tools", "ubench", "orient_naive.hip")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-o", path, src], check=True)
    L = C.CDLL(path)
    L.orient_naive_rot90.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
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


def orient_section(root, n, rounds, reps, naive_path):
    import numpy as np
    pkg, A = setup(root)
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    hip = Hip()
    NL = naive_lib(naive_path)
    L.dsvg_lane_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.dsvg_lane_stream.argtypes = [C.c_void_p]
    L.dsvg_lane_stream.restype = C.c_void_p
    L.dsvg_lane_sync.argtypes = [C.c_void_p]
    L.dsvg_lane_destroy.argtypes = [C.c_void_p]
    L.dsvg_orient_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.dsvg_orient_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.dsvg_orient_destroy.argtypes = [C.c_void_p]
    mem = pkg.Batch(pkg.make_encoder_cfg(64, 64, fmt), 1, 1)
    lane = C.c_void_p(None)
    passes = {}
    try:
        def dev(nbytes):
            p = C.c_void_p(None)
            assert L.dsvg_dev_alloc(mem.ctx, C.byref(p), nbytes) == 0
            return p

        def host(p, nbytes):
            out = np.zeros(nbytes, dtype=np.uint8)
            assert L.dsvg_dev_download(mem.ctx, out.ctypes.data, p, nbytes) == 0
            return out

        clip = A.gen_clip(W, H, fmt, 0xD0, 12, style=0)
        src = mem.upload(np.ascontiguousarray(np.tile(clip, (n // 12 + 1, 1))[:n]))
        out, plain, other = dev(n * FB), dev(n * FB), dev(n * FB)
        assert L.dsvg_lane_create(C.byref(lane), 0) == 0
        st = L.dsvg_lane_stream(lane)
        for code in (HFLIP, ROT180, ROT90):
            passes[code] = C.c_void_p(None)
            assert L.dsvg_orient_create(C.byref(passes[code]), 0, code, W, H, fmt) == 0

        def run(code):
            def fn():
                assert L.dsvg_orient_run(passes[code], st, src, n, out) == 0
            return fn

        def naive():
            assert NL.orient_naive_rot90(st, src, plain, W, H, 1, 1, n) == 0

        def copy():
            hip.d2d(other, out, n * FB, st)

        # the plain kernel writes the frames the pass writes (ROT90 runs last below, so `out` holds its result)
        run(ROT90)()
        naive()
        assert L.dsvg_lane_sync(lane) == 0
        assert np.array_equal(host(out, 2 * FB), host(plain, 2 * FB)), "the plain kernel and k_orient_tr disagree"
        fns = (("hflip", run(HFLIP)), ("rot180", run(ROT180)), ("rot90", run(ROT90)), ("naive", naive), ("copy", copy))
        t = {name: [] for name, _ in fns}
        for r in range(rounds + 1):
            for name, fn in fns:
                s = hip.timed(st, fn, reps)
                if r:                                    # (round 0 warms up)
                    t[name].append(s)
        assert L.dsvg_lane_sync(lane) == 0
    finally:
        if lane:
            L.dsvg_lane_sync(lane)
        for p in passes.values():
            if p:
                L.dsvg_orient_destroy(p)
        if lane:
            L.dsvg_lane_destroy(lane)
        mem.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    tbs = lambda s: 2 * n * FB / s / 1e12
    lines = ["%dx%d 4:2:0, %d pictures resident in HBM; device events around %d back-to-back enqueues on one stream, %d timed rounds after one" % (W, H, n, reps, rounds),
             "warm-up round, the five alternating.  Every one of them reads %d bytes and writes %d per call.  Measured %s." % (n * FB, n * FB, datetime.date.today().isoformat()),
             "k_orient_rows HFLIP:    %s; %.2f TB/s read + written" % (stats(t["hflip"]), tbs(med["hflip"])),
             "k_orient_rows ROT180:   %s; %.2f TB/s read + written" % (stats(t["rot180"]), tbs(med["rot180"])),
             "k_orient_tr ROT90:      %s; %.2f TB/s read + written" % (stats(t["rot90"]), tbs(med["rot90"])),
             "plain kernel ROT90:     %s; %.2f TB/s read + written" % (stats(t["naive"]), tbs(med["naive"])),
             "hipMemcpyAsync D2D:     %s; %.2f TB/s read + written" % (stats(t["copy"]), tbs(med["copy"])),
             "ratios (time): HFLIP / copy %.2f, ROT180 / copy %.2f, ROT90 / copy %.2f, ROT90 / plain kernel %.2f (plain kernel / copy %.2f)" % (
                 med["hflip"] / med["copy"], med["rot180"] / med["copy"], med["rot90"] / med["copy"], med["rot90"] / med["naive"], med["naive"] / med["copy"]),
             "per picture: HFLIP %.2f us, ROT180 %.2f us, ROT90 %.2f us, plain ROT90 %.2f us, copy %.2f us" % tuple(
                 med[k] * 1e6 / n for k in ("hflip", "rot180", "rot90", "naive", "copy")),
             "k_orient_tr is %s than the plain kernel in this run." % ("FASTER" if med["rot90"] < med["naive"] else "NOT faster")]
    return lines


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
    ap.add_argument("--root", default=HERE, help="the built tree of the project to measure (default: this one)")
    ap.add_argument("--naive", default=os.path.join(HERE, "tools", "ubench", "liborient_naive.so"), help="the plain kernel's shared library")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "orient_cost.txt"))
    a = ap.parse_args()
    lines = orient_section(os.path.abspath(a.root), a.frames, a.rounds, a.reps, a.naive)
    write_section(a.out, ("orient", "k_orient_rows and k_orient_tr against a device-to-device copy and a plain kernel (python tools/orient_cost.py)", lines))


if __name__ == "__main__":
    main()
