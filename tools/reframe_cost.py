#!/usr/bin/env python3
"""What the reframe pass and the line sums cost (dsv1_reframe_clip, dsv1_line_sums_clip, dsv1_batch_set_source_reframe;
csrc/k_reframe.hip), 1920x1080 4:2:0, on one MI355X.

profiles/reframe_cost.txt is kept in sections, each opened by a line "== name: title"; this tool rewrites the sections it measures
and leaves every other section as it finds it:

    python tools/reframe_cost.py [--frames 96] [--rounds 9]
        section "reframe": k_reframe on a device-resident clip, 2.39:1 window (0, 140, 1920, 800) -> 1920x800, against a
        hipMemcpyAsync device-to-device of the same OUTPUT bytes on the same stream, alternating, each timed with device events
        around `--reps` back-to-back enqueues.
        section "linesums": k_line_sums (with the zeroing of its column sums) over the same clip, per picture.
        section "batch": a host-fed batch step (4 sources x 12 frames, -gop12 -qp85 -rc_mode1, pinned host clip, encode() timed on
        the host) with the reframe set and fed the 1080p clip, against the same batch fed the pre-cut 1920x800 clip, alternating.
        section "off": a 1920x1080 batch with nothing set (8 sources x 12 frames, a held device clip), submit + collect timed on the
        host: median, min, max and the spread over the rounds.
    python tools/reframe_cost.py --only off --root OTHER_TREE --section off-parent
        the same measurement on another built tree of the project (the parent commit), written as section "off-parent": the
        feature off must agree with it within the spread both sections show.

Compulsory bytes of the reframe: one byte read per window sample, one byte written per canvas sample."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

HERE = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
W, H = 1920, 1080
WIN = (0, 140, 1920, 800)
OW, OH = 1920, 800
FB, OFB = W * H * 3 // 2, OW * OH * 3 // 2              # 4:2:0
HEAD = "Cost of the reframe pass and the line sums (csrc/k_reframe.hip); written by tools/reframe_cost.py, section by section"


def setup(root):
    import importlib
    sys.path.insert(0, os.path.join(root, "tests"))
    sys.path.insert(0, root)
    import _cabi as A
    assert A.frame_bytes(W, H, A.SUBSAMP_420) == FB
    return importlib.import_module("digital-subband-video-1_amd"), A


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


def kernel_sections(root, n, rounds, reps):
    import numpy as np
    pkg, A = setup(root)
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    hip = Hip()
    L.dsvg_lane_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.dsvg_lane_stream.argtypes = [C.c_void_p]
    L.dsvg_lane_stream.restype = C.c_void_p
    L.dsvg_lane_sync.argtypes = [C.c_void_p]
    L.dsvg_lane_destroy.argtypes = [C.c_void_p]
    L.dsvg_reframe_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(pkg.Reframe), C.c_int]
    L.dsvg_reframe_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.dsvg_reframe_destroy.argtypes = [C.c_void_p]
    L.dsvg_linesums_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]
    L.dsvg_linesums_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.dsvg_linesums_destroy.argtypes = [C.c_void_p]
    mem = pkg.Batch(pkg.make_encoder_cfg(64, 64, fmt), 1, 1)
    lane, rfp, lsp = C.c_void_p(None), C.c_void_p(None), C.c_void_p(None)
    try:
        def dev(nbytes):
            p = C.c_void_p(None)
            assert L.dsvg_dev_alloc(mem.ctx, C.byref(p), nbytes) == 0
            return p

        clip = A.gen_clip(W, H, fmt, 0xD0, 12, style=0)
        src = mem.upload(np.ascontiguousarray(np.tile(clip, (n // 12 + 1, 1))[:n]))
        out, other = dev(n * OFB), dev(n * OFB)
        rows, cols = dev(4 * n * H), dev(4 * n * W)
        rf = pkg.Reframe(W, H, WIN, (OW, OH))
        assert L.dsvg_lane_create(C.byref(lane), 0) == 0
        st = L.dsvg_lane_stream(lane)
        assert L.dsvg_reframe_create(C.byref(rfp), 0, C.byref(rf), fmt) == 0
        assert L.dsvg_linesums_create(C.byref(lsp), 0, W, H, fmt) == 0

        def reframe():
            assert L.dsvg_reframe_run(rfp, st, src, n, out) == 0

        def copy():
            hip.d2d(other, out, n * OFB, st)

        def sums():
            assert L.dsvg_linesums_run(lsp, st, src, n, rows, cols) == 0

        t = {"reframe": [], "copy": [], "sums": []}
        for r in range(rounds + 1):
            for name, fn in (("reframe", reframe), ("copy", copy), ("sums", sums)):
                s = hip.timed(st, fn, reps)
                if r:                                    # (round 0 warms up)
                    t[name].append(s)
        assert L.dsvg_lane_sync(lane) == 0
    finally:
        if lane:
            L.dsvg_lane_sync(lane)
        if rfp:
            L.dsvg_reframe_destroy(rfp)
        if lsp:
            L.dsvg_linesums_destroy(lsp)
        if lane:
            L.dsvg_lane_destroy(lane)
        mem.close()
    win_bytes = n * WIN[2] * WIN[3] * 3 // 2
    rfm, cpm, lsm = statistics.median(t["reframe"]), statistics.median(t["copy"]), statistics.median(t["sums"])
    a = ["%dx%d 4:2:0, %d pictures resident in HBM, window %s -> %dx%d; device events around %d back-to-back enqueues on one stream," % (W, H, n, WIN, OW, OH, reps),
         "%d timed rounds, the three alternating.  Bytes: %d read (the window) + %d written (the canvas) per call; the copy moves the" % (rounds, win_bytes, n * OFB),
         "same %d output bytes device to device (read + written)." % (n * OFB),
         "k_reframe:              %s; %.2f TB/s read + written" % (stats(t["reframe"]), (win_bytes + n * OFB) / rfm / 1e12),
         "hipMemcpyAsync D2D:     %s; %.2f TB/s read + written" % (stats(t["copy"]), 2 * n * OFB / cpm / 1e12),
         "ratio k_reframe / copy: %.2f (time); per picture %.2f us against %.2f us" % (rfm / cpm, rfm * 1e6 / n, cpm * 1e6 / n)]
    b = ["The same clip and stream: hipMemsetAsync of the column sums + k_line_sums over %d pictures (%d luma bytes read per call)." % (n, n * W * H),
         "k_line_sums:            %s; %.2f us per 1080p picture, %.2f TB/s of luma read" % (stats(t["sums"]), lsm * 1e6 / n, n * W * H / lsm / 1e12)]
    return a, b


def batch_section(root, rounds):
    import numpy as np
    pkg, A = setup(root)
    fmt, S, F = A.SUBSAMP_420, 4, 12
    clip = A.gen_clip(W, H, fmt, 0xD0, F, style=0)
    rf = pkg.Reframe(W, H, WIN, (OW, OH))
    cfg = pkg.make_encoder_cfg(OW, OH, fmt, qp=85, gop=12, rc_mode_cli=1)
    lib = pkg.lib()
    cut = np.zeros((F, OFB), dtype=np.uint8)
    for t in range(F):                                   # (the pre-cut clip, on the host: what a caller does today)
        y = clip[t, :W * H].reshape(H, W)[WIN[1]:WIN[1] + WIN[3]]
        u, v = (clip[t, W * H + k * (W // 2) * (H // 2):W * H + (k + 1) * (W // 2) * (H // 2)].reshape(H // 2, W // 2)[WIN[1] // 2:(WIN[1] + WIN[3]) // 2] for k in (0, 1))
        cut[t] = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])
    on, off = pkg.Batch(cfg, S, F), pkg.Batch(cfg, S, F)
    times = {True: [], False: []}
    try:
        on.set_source_reframe(rf)
        pin_on, pin_off = on.pinned((S, F, FB)), off.pinned((S, F, OFB))
        pin_on[...] = clip[None]
        pin_off[...] = cut[None]
        a, b_ = on.encode(pin_on), off.encode(pin_off)
        assert [bytes(x) for x in a] == [bytes(x) for x in b_], "the reframed batch does not code the pre-cut clip's streams"
        for r in range(rounds + 1):
            for which, b, pin in ((True, on, pin_on), (False, off, pin_off)):
                t0 = time.perf_counter()
                b.encode(pin)
                if r:
                    times[which].append(time.perf_counter() - t0)
    finally:
        on.close()
        off.close()
    m_on, m_off = statistics.median(times[True]), statistics.median(times[False])
    return ["Batches of %d sources x %d frames, canvas %dx%d 4:2:0, -gop12 -qp85 -rc_mode1, pinned host clips, encode() timed on the host, %d timed" % (S, F, OW, OH, rounds),
            "rounds, alternating; the streams of the two are the same (checked).  The reframed batch uploads %dx%d frames (%.0f %% more bytes over" % (W, H, 100.0 * (FB - OFB) / OFB),
            "the link) and runs the pass; the other is fed the clip a host has cut (the cutting itself is not timed).",
            "reframe set, fed 1080p:    %s" % stats(times[True]),
            "nothing set, fed pre-cut:  %s" % stats(times[False]),
            "difference: %+.3f ms per call, %+.2f %%" % ((m_on - m_off) * 1e3, 100 * (m_on - m_off) / m_off)]


def off_section(root, rounds):
    import numpy as np
    pkg, A = setup(root)
    fmt, S, F = A.SUBSAMP_420, 8, 12
    clip = A.gen_clip(W, H, fmt, 0xD0, F, style=0)
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, qp=85, gop=12, rc_mode_cli=1), S, F)
    ts = []
    try:
        dev = b.upload(np.ascontiguousarray(np.stack([clip] * S)))
        for r in range(rounds + 2):
            t0 = time.perf_counter()
            b.submit(dev, on_device=True, held=True)
            b.collect()
            if r > 1:
                ts.append(time.perf_counter() - t0)
    finally:
        b.close()
    return ["A batch of %d sources x %d frames, %dx%d 4:2:0, -gop12 -qp85 -rc_mode1, nothing set, a held device clip, submit + collect timed on" % (S, F, W, H),
            "the host, %d timed calls after two warm-up calls.  Tree: %s." % (rounds, "the one given with --root" if root != HERE else "this commit"),
            "per call: %s" % stats(ts)]


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
    ap.add_argument("--only", choices=["kernels", "batch", "off"], help="measure one group of sections (default: all)")
    ap.add_argument("--root", default=HERE, help="the built tree of the project to measure (default: this one)")
    ap.add_argument("--section", default="off", help="the name the `off` measurement is written under")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "reframe_cost.txt"))
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    cmd = "python tools/reframe_cost.py"
    if a.only in (None, "kernels"):
        ra, rb = kernel_sections(root, a.frames, a.rounds, a.reps)
        write_section(a.out, ("reframe", "k_reframe against a device-to-device copy (%s)" % cmd, ra))
        write_section(a.out, ("linesums", "k_line_sums per picture (%s)" % cmd, rb))
    if a.only in (None, "batch"):
        write_section(a.out, ("batch", "a host-fed batch step, reframed on the GPU against pre-cut (%s)" % cmd, batch_section(root, a.rounds)))
    if a.only in (None, "off"):
        extra = "" if a.section == "off" else " --only off --root <tree of the parent commit> --section %s" % a.section
        write_section(a.out, (a.section, "a batch with nothing set (%s%s)" % (cmd, extra), off_section(root, a.rounds)))


if __name__ == "__main__":
    main()
