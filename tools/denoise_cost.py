#!/usr/bin/env python3
"""What temporal noise reduction costs and buys (dsv1_denoise_clip, dsv1_batch_set_source_denoise; csrc/k_denoise.hip), 1920x1080
4:2:0, 96 frames.

profiles/denoise_cost.txt is kept in sections, each opened by a line "== name: title".  This tool rewrites the sections it measures
and leaves every other section (the bench.py record: kept by hand) exactly as it finds it:

    python tools/denoise_cost.py [--frames 96] [--rounds 9]
        section "host": a device-resident clip through the standalone pass, as ONE stream of 96 pictures and as 8 streams of 12 (the
        recursion runs along time: parallelism is samples x sources), beside dsv1_convert_clip of a same-sized planar 8-bit clip
        with padded pitches -- the existing pure one-read-one-write streaming pass -- in the same run, the settings alternating;
        each synchronous call timed on the host (stream creation and the launch included).
        section "batch": a batch of 8 sources x 12 frames at the headline's flags (-gop12 -qp85 -rc_mode1), encode() of a held
        device clip with the filter off and on, alternating: the per-call cost of the pass inside a session.
        section "benefit": a noisy synthetic clip (clean scene + Gaussian noise, sigma 2 and 4) coded at the headline's flags with
        the filter off and on: stream bytes, and the PSNR of both decoded clips against the CLEAN scene.
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/denoise_cost.py --only host --out DIR/host.txt
    python tools/denoise_cost.py --trace DIR/.../*_kernel_trace.csv
        section "kernels": the kernels' own times from the trace of such a run (no device needed for the second step).

Compulsory bytes of the pass: every picture read once and written once, 2 B per sample, plus the state (3 B per sample of a
picture) read and written once per call."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
W, H = 1920, 1080
FB = W * H * 3 // 2                                      # 4:2:0
HEAD = "Cost and benefit of temporal noise reduction (csrc/k_denoise.hip); written by tools/denoise_cost.py, section by section"
NAMES = ["convert planar, padded pitches (yardstick)", "denoise, 1 stream x %d", "denoise, 8 streams x %d"]


def passes(n):
    """(name, compulsory bytes of a call)"""
    return [(NAMES[0], 2 * FB * n), (NAMES[1] % n, 2 * FB * n + 6 * FB), (NAMES[2] % (n // 8), 2 * FB * n + 8 * 6 * FB)]


def table(times, n, unit, scale, per):
    ref = statistics.median(times[passes(n)[0][0]])
    lines = ["%-46s %10s %10s %14s %10s %12s" % ("pass", "median " + unit, "min " + unit, "bytes", per[0], "x yardstick")]
    for name, nbytes in passes(n):
        med = statistics.median(times[name])
        lines.append("%-46s %10.3f %10.3f %14d %10.2f %12.2f" % (name, med * scale, min(times[name]) * scale, nbytes, nbytes / med / per[1], med / ref))
    return lines


def setup():
    import importlib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import _cabi as A
    assert A.frame_bytes(W, H, A.SUBSAMP_420) == FB
    return importlib.import_module("digital-subband-video-1_amd"), A


def noisy_clip(A, n, sigma, seed=0xD0):
    """(clean, noisy) [n, FB]: the benchmark's synthetic scene and the same under Gaussian noise"""
    import numpy as np
    clean = A.gen_clip(W, H, A.SUBSAMP_420, seed, n, style=0)
    rng = np.random.default_rng(seed)
    noisy = np.empty_like(clean)
    for t in range(n):                                   # (frame by frame: the float copy of a whole clip is large)
        noisy[t] = np.clip(np.rint(clean[t] + sigma * rng.standard_normal(FB)), 0, 255).astype(np.uint8)
    return clean, noisy


def host_section(n, rounds):
    import ctypes as C
    import time

    import numpy as np
    pkg, A = setup()
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    padded = pkg.PixFormat(pkg.PIX_PLANAR, 8, 0, (W + 128, W // 2 + 64, W // 2 + 64))
    pfb = pkg.pix_frame_bytes(padded, W, H, fmt)
    mem = pkg.Batch(pkg.make_encoder_cfg(64, 64, fmt), 1, 1)
    try:
        def dev(nbytes):
            p = C.c_void_p(None)
            assert L.dsvg_dev_alloc(mem.ctx, C.byref(p), nbytes) == 0
            return p

        _, noisy = noisy_clip(A, 12, 2.0)
        src = mem.upload(np.ascontiguousarray(np.tile(noisy, (n // 12 + 1, 1))[:n]))
        raw = mem.upload(np.random.default_rng(2).integers(0, 256, n * pfb, dtype=np.uint8))
        out = dev(n * FB)
        state = dev(3 * FB)
        dn = pkg.Denoise(24, 24)
        pkg.denoise_clip(src, W, H, fmt, dn, n=1, out=out, state_out=state)
        # 8 streams of n / 8: the standalone call takes one stream, so this figure comes from a session's filter object (section "batch"
        # has a whole call)
        try:
            d8, lane = C.c_void_p(None), C.c_void_p(None)
            L.dsvg_lane_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
            L.dsvg_lane_stream.argtypes = [C.c_void_p]
            L.dsvg_lane_stream.restype = C.c_void_p
            L.dsvg_lane_sync.argtypes = [C.c_void_p]
            L.dsvg_lane_destroy.argtypes = [C.c_void_p]
            L.dsvg_denoise_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(pkg.Denoise), C.c_int, C.c_int]
            L.dsvg_denoise_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
            L.dsvg_denoise_destroy.argtypes = [C.c_void_p]
            assert L.dsvg_lane_create(C.byref(lane), 0) == 0
            assert L.dsvg_denoise_create(C.byref(d8), 0, W, H, fmt, C.byref(dn), 8, 1) == 0
            st = L.dsvg_lane_stream(lane)

            def eight():
                assert L.dsvg_denoise_run(d8, st, src, n // 8, out) == 0 and L.dsvg_lane_sync(lane) == 0

            fns = [lambda: pkg.convert_clip(raw, padded, W, H, fmt, n=n, out=out),
                   lambda: pkg.denoise_clip(src, W, H, fmt, dn, state=state, n=n, out=out, state_out=state), eight]
            times = {name: [] for name, _ in passes(n)}
            for r in range(rounds + 1):
                for (name, _), fn in zip(passes(n), fns):
                    t0 = time.perf_counter()
                    fn()
                    if r:                                # (round 0 warms up)
                        times[name].append(time.perf_counter() - t0)
        finally:
            if lane:
                L.dsvg_lane_sync(lane)                   # (the filter's kernels read what its destroy frees)
            if d8:
                L.dsvg_denoise_destroy(d8)
            if lane:
                L.dsvg_lane_destroy(lane)
    finally:
        mem.close()
    return ["%dx%d 4:2:0, %d pictures resident in HBM, luma = chroma = 24, %d timed rounds, the settings alternating.  The standalone calls" % (W, H, n, rounds),
            "create and destroy their stream and event, which is most of their time; the 8-stream pass is a session's (no creation)."] + \
        table(times, n, "ms", 1e3, ("GB/s", 1e9))


def kernel_section(path, n):
    """the kernels' own times from a rocprofv3 --kernel-trace CSV of one `--only host` run of this tool: per round the yardstick's
    launches, k_denoise for one stream, k_denoise for 8 streams (Grid_Size_Y 1 and 8 workgroups); the warm-up round is dropped"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
    dn = [r for r in rows if "k_denoise" in r["Kernel_Name"]][1:]                      # (the first launch made the state)
    conv = [r for r in rows if "k_pixfmt" in r["Kernel_Name"]]
    rounds = len(dn) // 2
    if rounds < 2 or len(dn) != 2 * rounds or len(conv) % rounds:
        raise SystemExit("%s: %d k_denoise and %d k_pixfmt launches: not a trace of one run of this tool" % (path, len(dn), len(conv)))
    per = len(conv) // rounds
    names = [p[0] for p in passes(n)]
    times = {names[0]: [sum(dur(r) for r in conv[k * per:(k + 1) * per]) for k in range(1, rounds)],
             names[1]: [dur(dn[2 * k]) for k in range(1, rounds)], names[2]: [dur(dn[2 * k + 1]) for k in range(1, rounds)]}
    k0 = dn[0]
    regs = ", ".join("%s %s" % (c, k0[c]) for c in ("VGPR_Count", "Accum_VGPR_Count", "SGPR_Count", "LDS_Block_Size", "Scratch_Size") if c in k0)
    return ["The kernels' own time per call under rocprofv3 --kernel-trace (%d timed rounds, the warm-up round dropped; the yardstick is" % (rounds - 1),
            "k_pixfmt<planar, 8 bit>, %d launch(es) per call).  k_denoise as dispatched: %s." % (per, regs)] + table(times, n, "us", 1e6, ("TB/s", 1e12))


def batch_section(rounds):
    import time

    import numpy as np
    pkg, A = setup()
    fmt, S, F = A.SUBSAMP_420, 8, 12
    _, noisy = noisy_clip(A, F, 2.0)
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, qp=85, gop=12, rc_mode_cli=1), S, F)
    times = {False: [], True: []}
    try:
        clip = b.upload(np.ascontiguousarray(np.stack([noisy] * S)))
        for r in range(rounds + 1):
            for on in (False, True):
                b.set_source_denoise(pkg.Denoise(24, 24) if on else None)
                b.submit(clip, on_device=True, held=True)             # (a first call after the setter: every source starts)
                b.collect()
                t0 = time.perf_counter()
                b.submit(clip, on_device=True, held=True)
                b.collect()
                if r:
                    times[on].append(time.perf_counter() - t0)
    finally:
        b.close()
    off, on = statistics.median(times[False]), statistics.median(times[True])
    return ["A batch of %d sources x %d frames, %dx%d 4:2:0, -gop12 -qp85 -rc_mode1, a held device clip, submit + collect timed on the host," % (S, F, W, H),
            "%d timed rounds, the filter off and on (luma = chroma = 24) alternating; the timed call continues the state of the call before." % rounds,
            "filter off: median %.3f ms, min %.3f ms per call" % (off * 1e3, min(times[False]) * 1e3),
            "filter on:  median %.3f ms, min %.3f ms per call" % (on * 1e3, min(times[True]) * 1e3),
            "the pass inside a call: %+.3f ms, %+.2f %% of the call (%d pictures: %.2f us per picture)" % ((on - off) * 1e3, 100 * (on - off) / off, S * F, (on - off) * 1e6 / (S * F))]


def benefit_section(n):
    import numpy as np
    pkg, A = setup()
    fmt, F = A.SUBSAMP_420, 12
    lines = ["%dx%d 4:2:0, %d frames in calls of %d, -gop12 -qp85 -rc_mode1 (the headline's flags); the synthetic scene of the benchmark plus" % (W, H, n, F),
             "Gaussian noise; PSNR (all planes together) of the decoded stream against the CLEAN scene, and of the noisy source itself.",
             "%-6s %-14s %12s %12s %14s %14s" % ("sigma", "filter", "stream bytes", "bytes ratio", "PSNR dB clean", "source dB")]

    def psnr(a, b):
        d = a.astype(np.float64) - b.astype(np.float64)
        return 10 * np.log10(255.0 ** 2 / (d * d).mean())

    for sigma, T in ((2.0, 24), (4.0, 48)):
        clean, noisy = noisy_clip(A, n, sigma)
        base = None
        for dn in (None, pkg.Denoise(T, T)):
            b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, qp=85, gop=12, rc_mode_cli=1), 1, F)
            try:
                b.set_source_denoise(dn)
                stream = b"".join(bytes(b.encode(noisy[None, k:k + F])[0]) for k in range(0, n, F))
            finally:
                b.close()
            rec = np.stack(A.orc_decode(stream, W, H, fmt))[:n]        # (the oracle's decoder: the reconstruction is the same on every decoder)
            base = base or len(stream)
            lines.append("%-6.1f %-14s %12d %12.3f %14.2f %14.2f" % (sigma, "off" if dn is None else "%d / %d" % (T, T), len(stream), len(stream) / base,
                                                                     psnr(rec, clean), psnr(noisy, clean)))
    return lines


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
    ap.add_argument("--only", choices=["host", "batch", "benefit"], help="measure one section (default: all three)")
    ap.add_argument("--trace", help="a rocprofv3 kernel-trace CSV of an `--only host` run of this tool: write section \"kernels\" from it and run nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_cost.txt"))
    a = ap.parse_args()
    if a.trace:
        new = [("kernels", "the kernels' own times (python tools/denoise_cost.py --trace)", kernel_section(a.trace, a.frames))]
    else:
        new = []
        for name, title, fn in (("host", "host-timed synchronous calls (python tools/denoise_cost.py)", lambda: host_section(a.frames, a.rounds)),
                                ("batch", "the pass inside a batch's call (python tools/denoise_cost.py)", lambda: batch_section(a.rounds)),
                                ("benefit", "what the encoder saves (python tools/denoise_cost.py)", lambda: benefit_section(a.frames))):
            if a.only in (None, name):
                new.append((name, title, fn()))
                secs = read_sections(a.out)              # (written section by section: a later one that fails loses nothing)
                secs = [new[-1] if s[0] == name else s for s in secs] if name in [s[0] for s in secs] else secs + [new[-1]]
                write_sections(a.out, secs)
                print("\n".join(new[-1][2]))
        return
    secs = read_sections(a.out)
    for sec in new:
        secs = [sec if s[0] == sec[0] else s for s in secs] if sec[0] in [s[0] for s in secs] else secs + [sec]
        print("\n".join(sec[2]))
    write_sections(a.out, secs)


if __name__ == "__main__":
    main()
