#!/usr/bin/env python3
"""What deinterlacing costs (dsv1_deinterlace_clip, csrc/k_deint.hip).  A device-resident 1920x1080 4:2:0 clip of 96 frames through
the standalone pass in both modes, and -- the yardstick, in the same run -- dsv1_convert_clip of a same-sized planar 8-bit clip with
padded pitches: the existing pure one-read-one-write streaming pass.  The settings ALTERNATE within the run (--rounds rounds over
all of them after one warm-up round).

profiles/deint_cost.txt is kept in sections, each opened by a line "== name: title".  This tool rewrites the sections it measures
and leaves every other section (the counter passes, the bench.py record: kept by hand) exactly as it finds it:

    python tools/deint_cost.py [--frames 96] [--rounds 9]
        runs the passes and times each synchronous call on the host (stream creation and the launch included): section "host".
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/deint_cost.py --out DIR/host.txt
    python tools/deint_cost.py --trace DIR/.../*_kernel_trace.csv
        the kernels' own times from the trace of such a run (no device needed for the second step): section "kernels".

Reported: median and minimum time, compulsory bytes (cur + prv read, output written: 3 B per output sample at frame rate, 2 at field
rate; 2 for the yardstick) per second, and the ratio of the times to the yardstick's."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
W, H = 1920, 1080
FB = W * H * 3 // 2                                      # 4:2:0
HEAD = "Cost of deinterlacing (dsv1_deinterlace_clip, csrc/k_deint.hip); written by tools/deint_cost.py, section by section"


def passes(n):
    """(name, compulsory bytes of a call, output pictures)"""
    return [("convert planar, padded pitches (yardstick)", 2 * FB * n, n), ("deinterlace FRAME", 3 * FB * n, n), ("deinterlace FIELD", 2 * FB * 2 * n, 2 * n)]


def table(times, n, unit, scale, per):
    """times: {pass name: [seconds]} -> lines; bytes per second in `per` (name, divisor)"""
    ref = statistics.median(times[passes(n)[0][0]])
    lines = ["%-46s %9s %10s %10s %14s %10s %12s" % ("pass", "pictures", "median " + unit, "min " + unit, "bytes", per[0], "x yardstick")]
    for name, nbytes, pics in passes(n):
        med = statistics.median(times[name])
        lines.append("%-46s %9d %10.3f %10.3f %14d %10.2f %12.2f" % (name, pics, med * scale, min(times[name]) * scale, nbytes, nbytes / med / per[1], med / ref))
    return lines


def host_section(n, rounds):
    import ctypes as C
    import importlib
    import time

    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import _cabi as A
    fmt = A.SUBSAMP_420
    assert A.frame_bytes(W, H, fmt) == FB
    pkg = importlib.import_module("digital-subband-video-1_amd")
    L = pkg.lib()
    padded = pkg.PixFormat(pkg.PIX_PLANAR, 8, 0, (W + 128, W // 2 + 64, W // 2 + 64))
    pfb = pkg.pix_frame_bytes(padded, W, H, fmt)
    mem = pkg.Batch(pkg.make_encoder_cfg(64, 64, fmt), 1, 1)
    try:
        def dev(nbytes):
            p = C.c_void_p(None)
            assert L.dsvg_dev_alloc(mem.ctx, C.byref(p), nbytes) == 0
            return p

        # interlaced-looking content: a few distinct frames of moving pictures, repeated (the pass's time does not depend on content
        # beyond which directions win; noise would make every direction's test fail the same way)
        few = A.gen_clip(W, H, fmt, 0xDE1, 8, style=1)
        src = mem.upload(np.ascontiguousarray(np.tile(few, (n // 8 + 1, 1))[:n]))
        raw = mem.upload(np.random.default_rng(2).integers(0, 256, n * pfb, dtype=np.uint8))
        prev = mem.upload(few[7])
        out = dev(2 * n * FB)
        frame, field = pkg.Deint(pkg.DEINT_FRAME, 1), pkg.Deint(pkg.DEINT_FIELD, 1)
        fns = [lambda: pkg.convert_clip(raw, padded, W, H, fmt, n=n, out=out),
               lambda: pkg.deinterlace_clip(src, W, H, fmt, frame, prev=prev, n=n, out=out),
               lambda: pkg.deinterlace_clip(src, W, H, fmt, field, prev=prev, n=n, out=out)]
        times = {name: [] for name, _, _ in passes(n)}
        for r in range(rounds + 1):
            for (name, _, _), fn in zip(passes(n), fns):
                t0 = time.perf_counter()
                fn()
                if r:                                    # (round 0 warms up)
                    times[name].append(time.perf_counter() - t0)
    finally:
        mem.close()
    return ["%dx%d 4:2:0, %d frames resident in HBM, %d timed rounds, the settings alternating.  Each call creates and destroys its stream" % (W, H, n, rounds),
            "and event, which is most of these times: what a caller of the standalone entry point waits, not what the kernels take."] + \
        table(times, n, "ms", 1e3, ("GB/s", 1e9))


def kernel_section(path, n):
    """the kernels' own times from a rocprofv3 --kernel-trace CSV of one run of this tool: the launches in time order are, per round,
    the yardstick's, k_deint at frame rate, k_deint at field rate; the warm-up round is dropped"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
    di = [r for r in rows if "k_deint" in r["Kernel_Name"]]
    conv = [r for r in rows if "k_pixfmt" in r["Kernel_Name"]]
    rounds = len(di) // 2
    if rounds < 2 or len(di) != 2 * rounds or len(conv) % rounds:
        raise SystemExit("%s: %d k_deint and %d k_pixfmt launches: not a trace of one run of this tool" % (path, len(di), len(conv)))
    if "Grid_Size_Y" in di[0]:                           # (a field-rate launch has twice the pictures of the frame-rate one before it)
        assert all(int(di[2 * k + 1]["Grid_Size_Y"]) == 2 * int(di[2 * k]["Grid_Size_Y"]) for k in range(rounds)), "k_deint launches out of order"
    per = len(conv) // rounds
    names = [p[0] for p in passes(n)]
    times = {names[0]: [sum(dur(r) for r in conv[k * per:(k + 1) * per]) for k in range(1, rounds)],
             names[1]: [dur(di[2 * k]) for k in range(1, rounds)], names[2]: [dur(di[2 * k + 1]) for k in range(1, rounds)]}
    k0 = di[0]
    regs = ", ".join("%s %s" % (c, k0[c]) for c in ("VGPR_Count", "Accum_VGPR_Count", "SGPR_Count", "LDS_Block_Size", "Scratch_Size") if c in k0)
    return ["The kernels' own time per call under rocprofv3 --kernel-trace (%d timed rounds, the warm-up round dropped; the yardstick is" % (rounds - 1),
            "k_pixfmt<planar, 8 bit>, %d launch(es) per call).  k_deint as dispatched: %s." % (per, regs)] + table(times, n, "us", 1e6, ("TB/s", 1e12))


def read_sections(path):
    """[(name, title, [lines])] of a sectioned file; [] if there is none"""
    secs = []
    if os.path.exists(path):
        for line in open(path).read().splitlines():
            if line.startswith("== "):
                name, _, title = line[3:].partition(":")
                secs.append((name.strip(), title.strip(), []))
            elif secs:
                secs[-1][2].append(line)
    return secs


def write_sections(path, secs):
    with open(path, "w") as f:
        f.write(HEAD + "\n")
        for name, title, lines in secs:
            while lines and not lines[-1].strip():
                lines = lines[:-1]
            f.write("\n== %s: %s\n%s\n" % (name, title, "\n".join(lines)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--trace", help="a rocprofv3 kernel-trace CSV of a run of this tool: write section \"kernels\" from it and run nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deint_cost.txt"))
    a = ap.parse_args()
    if a.trace:
        new = ("kernels", "the kernels' own times (python tools/deint_cost.py --trace)", kernel_section(a.trace, a.frames))
    else:
        new = ("host", "host-timed synchronous calls (python tools/deint_cost.py)", host_section(a.frames, a.rounds))
    secs = read_sections(a.out)
    if new[0] in [s[0] for s in secs]:
        secs = [new if s[0] == new[0] else s for s in secs]
    else:                                                # (the tool's sections lead, the hand-kept ones follow)
        at = 0 if new[0] == "host" else int(bool(secs) and secs[0][0] == "host")
        secs.insert(at, new)
    write_sections(a.out, secs)
    print("\n".join(new[2]))


if __name__ == "__main__":
    main()
