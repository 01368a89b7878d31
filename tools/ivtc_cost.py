#!/usr/bin/env python3
"""What the inverse telecine costs (dsv1_batch_set_source_ivtc, dsv1_ivtc_clip; csrc/k_ivtc.hip), 1920x1080 4:2:0, on one MI355X.

profiles/ivtc_cost.txt is kept in sections, each opened by a line "== name: title"; this tool rewrites the sections it measures and
leaves every other section as it finds it:

    python tools/ivtc_cost.py [--sources 4] [--cycles 3] [--rounds 9] [--reps 10]
        section "pass": the whole pass of a session call (dsvg_ivtc_run: the zeroing of its tables, k_field_metrics, k_ivtc_match,
        k_ivtc_dup, k_ivtc_pick, k_ivtc_weave, k_ivtc_keep) over a device-resident telecined clip of `sources` x 5 `cycles` frames,
        against a hipMemcpyAsync device-to-device of the clip's INPUT bytes on the same stream, alternating, each timed with device
        events around `reps` back-to-back enqueues.  The result is checked against the film frames first.
    rocprofv3 --kernel-trace --stats -d DIR -o ivtc -- python tools/ivtc_cost.py --only pass --out /dev/null
    python tools/ivtc_cost.py --kernel-stats DIR/.../ivtc_kernel_stats.csv [--sources 4] [--cycles 3]
        section "kernels": each kernel's mean time per launch from the profiler's statistics (a run of its own: tracing slows the
        host, so the figures of section "pass" are taken without it) and the rate at which it moves the bytes its algorithm needs.
    python tools/ivtc_cost.py --bench RESULT.json --section bench | bench-parent
        the headline of `bench.py --gpus 1` (its JSON result line, kept in a file) with the pass off, of this commit and of the
        parent commit, run alternating on the same machine: the feature off must agree with the parent within their spread.

Bytes the algorithm needs, per input frame (L = one luma, fb = one frame = 1.5 L at 4:2:0): k_field_metrics reads cur and prv, 2 L;
k_ivtc_dup reads two woven lumas, 2 L; k_ivtc_weave reads and writes 0.8 fb; k_ivtc_keep, once per source and call, reads and writes
fb + L."""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys

HERE = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
W, H = 1920, 1080
LUMA = W * H
FB = LUMA * 3 // 2                                         # 4:2:0
HEAD = "Cost of the inverse telecine (csrc/k_ivtc.hip); written by tools/ivtc_cost.py, section by section"


def setup(root):
    import importlib
    sys.path.insert(0, os.path.join(root, "tests"))
    sys.path.insert(0, root)
    import _cabi as A
    import _ivtc as I
    assert A.frame_bytes(W, H, A.SUBSAMP_420) == FB
    return importlib.import_module("digital-subband-video-1_amd"), A, I


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


def kernel_bytes(S, nin):
    """bytes each kernel's algorithm needs per LAUNCH of a call of S sources x nin frames (k_ivtc_match and k_ivtc_pick read tables only)"""
    nout = nin // 5 * 4
    return {"k_field_metrics": 2 * LUMA * S * nin, "k_ivtc_dup": 2 * LUMA * S * nin, "k_ivtc_weave": 2 * FB * S * nout,
            "k_ivtc_keep": 2 * (FB + LUMA) * S}


def pass_section(root, S, cycles, rounds, reps):
    import numpy as np
    pkg, A, I = setup(root)
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    hip = Hip()
    L.dsvg_lane_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.dsvg_lane_stream.argtypes = [C.c_void_p]
    L.dsvg_lane_stream.restype = C.c_void_p
    L.dsvg_lane_sync.argtypes = [C.c_void_p]
    L.dsvg_lane_destroy.argtypes = [C.c_void_p]
    L.dsvg_ivtc_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(pkg.Ivtc), C.c_int, C.c_int, C.c_int]
    L.dsvg_ivtc_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dsvg_ivtc_reset.argtypes = [C.c_void_p, C.c_int]
    L.dsvg_ivtc_destroy.argtypes = [C.c_void_p]
    nin, nout = 5 * cycles, 4 * cycles
    mem = pkg.Batch(pkg.make_encoder_cfg(64, 64, fmt), 1, 1)
    lane, ivp = C.c_void_p(None), C.c_void_p(None)
    try:
        def dev(nbytes):
            p = C.c_void_p(None)
            assert L.dsvg_dev_alloc(mem.ctx, C.byref(p), nbytes) == 0
            return p

        films = [I.film_frames(W, H, fmt, nout, 0xC0 + s) for s in range(S)]
        clips = [I.telecine(f, W, H, fmt, 1, s)[0] for s, f in enumerate(films)]
        src = mem.upload(np.ascontiguousarray(np.stack(clips)))
        out, other = dev(S * nout * FB), dev(S * nin * FB)
        iv = pkg.Ivtc(1, 0)
        assert L.dsvg_lane_create(C.byref(lane), 0) == 0
        st = L.dsvg_lane_stream(lane)
        assert L.dsvg_ivtc_create(C.byref(ivp), 0, W, H, fmt, C.byref(iv), S, nin, 1) == 0

        def ivtc():
            assert L.dsvg_ivtc_run(ivp, st, src, out) == 0

        def copy():
            hip.d2d(other, src, S * nin * FB, st)

        # what is timed gives back the film frames
        ivtc()
        assert L.dsvg_lane_sync(lane) == 0
        got = np.zeros((S, nout, FB), dtype=np.uint8)
        assert L.dsvg_dev_download(mem.ctx, got.ctypes.data, out, got.nbytes) == 0
        assert np.array_equal(got, np.stack(films)), "the pass does not give back the film frames"
        assert L.dsvg_ivtc_reset(ivp, -1) == 0
        t = {"ivtc": [], "copy": []}
        for r in range(rounds + 1):
            for name, fn in (("ivtc", ivtc), ("copy", copy)):
                s = hip.timed(st, fn, reps)
                if r:                                    # (round 0 warms up; from its second call on every source has a state)
                    t[name].append(s)
        assert L.dsvg_lane_sync(lane) == 0
    finally:
        if lane:
            L.dsvg_lane_sync(lane)
        if ivp:
            L.dsvg_ivtc_destroy(ivp)
        if lane:
            L.dsvg_lane_destroy(lane)
        mem.close()
    im, cm = statistics.median(t["ivtc"]), statistics.median(t["copy"])
    need = sum(kernel_bytes(S, nin).values())
    return ["%dx%d 4:2:0, %d sources x %d telecined frames resident in HBM -> %d film frames each (checked); device events around %d" % (W, H, S, nin, nout, reps),
            "back-to-back enqueues on one stream, %d timed rounds, the two alternating.  The copy moves the clip's %d input bytes" % (rounds, S * nin * FB),
            "device to device (read + written); the pass's algorithm needs %d bytes read + written per call." % need,
            "inverse telecine:       %s; %.2f TB/s of the bytes it needs" % (stats(t["ivtc"]), need / im / 1e12),
            "hipMemcpyAsync D2D:     %s; %.2f TB/s read + written" % (stats(t["copy"]), 2 * S * nin * FB / cm / 1e12),
            "ratio pass / copy:      %.2f (time); per input frame %.2f us against %.2f us" % (im / cm, im * 1e6 / (S * nin), cm * 1e6 / (S * nin))]


def kernels_section(path, S, cycles):
    need = kernel_bytes(S, 5 * cycles)
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"].split("(")[0].strip()
            if name.startswith(("k_field_metrics", "k_ivtc_")):
                rows[name] = (int(r["Calls"]), float(r["AverageNs"]))
    if not rows:
        raise SystemExit("%s holds no k_ivtc kernel" % path)
    out = ["rocprofv3 --kernel-trace --stats over `tools/ivtc_cost.py --only pass`, %d sources x %d frames per call, %dx%d 4:2:0: mean time" % (S, 5 * cycles, W, H),
           "per launch, and the rate at which the kernel moves the bytes its algorithm needs (the two table kernels read a few hundred bytes)."]
    for name in ("k_field_metrics", "k_ivtc_match", "k_ivtc_dup", "k_ivtc_pick", "k_ivtc_weave", "k_ivtc_keep"):
        if name in rows:
            calls, ns = rows[name]
            rate = "  %.2f TB/s" % (need[name] / ns / 1e3) if name in need else ""
            out.append("%-16s %5d launches, %9.2f us each%s" % (name, calls, ns / 1e3, rate))
    return out


def bench_section(path):
    """every JSON result line the file holds (one per run, in the order they ran)"""
    out = []
    for line in open(path).read().splitlines():
        line = line.strip()
        if line.startswith("{") and line.endswith("}"):
            try:
                res = json.loads(line)
            except ValueError:
                continue
            out.append("run %d: %s %s, %s ms per step (steps %s, warmup %s, %s GPU)" % (len(out) + 1, res.get("value"), res.get("unit"), res.get("ms_per_step"),
                                                                                     res.get("steps"), res.get("warmup"), res.get("n_gpus")))
    if not out:
        raise SystemExit("%s holds no JSON result line" % path)
    return ["%s; the runs of the two commits alternated on one machine, the parent's first." % "bench.py --gpus 1 --steps 20 --warmup 5"] + out


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
    print("== %s\n%s" % (sec[0], "\n".join(sec[2])))
    if path == os.devnull:
        return
    secs = read_sections(path)
    secs = [sec if s[0] == sec[0] else s for s in secs] if sec[0] in [s[0] for s in secs] else secs + [sec]
    with open(path, "w") as f:
        f.write(HEAD + "\n")
        for name, title, lines in secs:
            while lines and not lines[-1].strip():
                lines = lines[:-1]
            f.write("\n== %s: %s\n%s\n" % (name, title, "\n".join(lines)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=3, help="cycles of 5 frames per source and call (3: frames_per_call 12)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["pass"], help="measure one section (default: pass, unless --kernel-stats or --bench is given)")
    ap.add_argument("--kernel-stats", metavar="CSV", help="rocprofv3's kernel statistics of a run of `--only pass`: writes section kernels")
    ap.add_argument("--bench", metavar="FILE", help="a file that holds bench.py's JSON result line: writes section --section")
    ap.add_argument("--section", default="bench", help="the name the --bench section is written under (bench, bench-parent)")
    ap.add_argument("--root", default=HERE, help="the built tree of the project to measure (default: this one)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ivtc_cost.txt"))
    a = ap.parse_args()
    cmd = "python tools/ivtc_cost.py"
    if a.kernel_stats:
        write_section(a.out, ("kernels", "each kernel, from the profiler (%s --kernel-stats CSV)" % cmd, kernels_section(a.kernel_stats, a.sources, a.cycles)))
    elif a.bench:
        what = "this commit" if a.section == "bench" else "the parent commit"
        write_section(a.out, (a.section, "bench.py --gpus 1 with the pass off, %s (%s --bench FILE --section %s)" % (what, cmd, a.section), bench_section(a.bench)))
    else:
        write_section(a.out, ("pass", "the whole pass against a device-to-device copy of its input (%s)" % cmd,
                              pass_section(os.path.abspath(a.root), a.sources, a.cycles, a.rounds, a.reps)))


if __name__ == "__main__":
    main()
