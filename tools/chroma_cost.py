#!/usr/bin/env python3
"""What chroma resampling in the source and output passes costs (dsv1_convert_clip_sub, dsv1_decbatch_set_output_format_up;
csrc/k_pixfmt.hip, csrc/k_pixout.hip).  1920x1080, one box, one run, the settings alternating within it.
  section "in":  a UYVY 4:2:2 clip held in HBM to planar 4:2:0 with the one call, against the two calls it replaces --
                 dsv1_convert_clip to planar 4:2:2, then dsv1_export_clip of that to planar 4:2:0 through an intermediate clip;
                 each synchronous call timed on the host (stream creation and the launch included: the two calls pay them twice).
                 Compulsory bytes of the result: the UYVY frames read once, the 4:2:0 frames written once.
  section "out": dsv1_decbatch_decode per call, --streams streams of one 1080p 4:2:0 GOP, device output: UYVY with linear
                 upsampling against NV12, a decoder of each alive, alternating call by call.
Writes profiles/chroma_resample_cost.txt.
    python tools/chroma_cost.py [--frames 24] [--streams 16] [--rounds 9]"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import _cabi as A  # noqa: E402

W, H, GOP, QP = 1920, 1080, 12, 85
S422, S420 = A.SUBSAMP_422, A.SUBSAMP_420


def in_section(pkg, n, rounds):
    L = pkg.lib()
    uyvy, planar = pkg.PixFormat(pkg.PIX_PACKED_UYVY), pkg.PixFormat()
    raw_fb, mid_fb, out_fb = 2 * W * H, A.frame_bytes(W, H, S422), A.frame_bytes(W, H, S420)
    mem = pkg.Batch(pkg.make_encoder_cfg(64, 64, S420), 1, 1)
    try:
        def dev(nbytes):
            p = C.c_void_p(None)
            assert L.dsvg_dev_alloc(mem.ctx, C.byref(p), nbytes) == 0
            return p

        raw = mem.upload(np.random.default_rng(1).integers(0, 256, n * raw_fb, dtype=np.uint8))
        mid, out, out2 = dev(n * mid_fb), dev(n * out_fb), dev(n * out_fb)

        def fused():
            pkg.convert_clip(raw, uyvy, W, H, S420, n=n, out=out, src_fmt=S422)

        def two():
            pkg.convert_clip(raw, uyvy, W, H, S422, n=n, out=mid)
            pkg.export_clip(mid, W, H, S422, planar, S420, n=n, out=out2)

        runs = [("one call: dsv1_convert_clip_sub", fused), ("two calls: dsv1_convert_clip + dsv1_export_clip", two)]
        ms = {name: [] for name, _ in runs}
        for r in range(rounds + 1):
            for name, fn in runs:
                t0 = time.perf_counter()
                fn()
                if r:                                    # (round 0 warms up)
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        a, b = np.zeros(n * out_fb, dtype=np.uint8), np.zeros(n * out_fb, dtype=np.uint8)
        mem.sync()
        assert L.dsvg_dev_download(mem.ctx, a.ctypes.data, out, a.nbytes) == 0 and L.dsvg_dev_download(mem.ctx, b.ctypes.data, out2, b.nbytes) == 0
        assert np.array_equal(a, b), "the one call and the two calls differ"
    finally:
        mem.close()
    nbytes = n * (raw_fb + out_fb)
    ref = statistics.median(ms[runs[1][0]])
    lines = ["UYVY 4:2:2 -> planar 4:2:0, %dx%d, %d frames held in HBM, %d timed rounds after one warm-up, the settings alternating; the results" % (W, H, n, rounds),
             "are the same bytes.  Host-timed synchronous calls (each creates and destroys its stream and event).",
             "%-50s %10s %10s %14s %8s %12s" % ("setting", "median ms", "min ms", "bytes", "GB/s", "x two calls")]
    for name, _ in runs:
        med = statistics.median(ms[name])
        lines.append("%-50s %10.3f %10.3f %14d %8.1f %12.3f" % (name, med, min(ms[name]), nbytes, nbytes / med / 1e6, med / ref))
    return lines


def out_section(pkg, S, rounds):
    clip = A.gen_clip(W, H, S420, 0xC405, GOP, style=2)
    packets = A.split_packets(pkg.encode_clip(clip, W, H, S420, qp=QP, gop=GOP, rc_mode_cli=1))
    settings = [("NV12 (dsv1_decbatch_set_output_format)", lambda d: d.set_output_format(pkg.PixFormat(pkg.PIX_SEMIPLANAR_UV)), A.frame_bytes(W, H, S420)),
                ("UYVY, linear (dsv1_decbatch_set_output_format_up)", lambda d: d.set_output_format(pkg.PixFormat(pkg.PIX_PACKED_UYVY), S422, upsample=pkg.CHROMA_LINEAR), 2 * W * H)]
    ms = {name: [] for name, _, _ in settings}
    for r in range(rounds + 1):
        ds = []
        try:
            for name, setter, fb in settings:
                d = pkg.DecBatch(W, H, S420, S)
                ds.append(d)
                setter(d)
                assert d.frame_bytes == fb
            calls = {name: [] for name, _, _ in settings}
            for p in packets:
                for (name, _, _), d in zip(settings, ds):
                    t0 = time.perf_counter()
                    d.decode([p] * S, on_device=True)
                    d.sync()
                    if p[5] & 4:
                        calls[name].append((time.perf_counter() - t0) * 1e3)
            if r:
                for name in calls:
                    ms[name].append(statistics.median(calls[name]))
        finally:
            for d in ds:
                d.close()
    ref = statistics.median(ms[settings[0][0]])
    lines = ["dsv1_decbatch_decode of %d streams of one %dx%d 4:2:0 GOP (%d pictures, -qp%d), device output, decode + sync timed on the host per" % (S, W, H, GOP, QP),
             "call; a decoder of each setting alive, alternating call by call; per round the median over the GOP's calls, %d rounds after one warm-up." % rounds,
             "%-52s %12s %12s %16s %10s" % ("output", "median ms", "min ms", "out bytes / call", "x NV12")]
    for name, _, fb in settings:
        med = statistics.median(ms[name])
        lines.append("%-52s %12.3f %12.3f %16d %10.3f" % (name, med, min(ms[name]), S * fb, med / ref))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chroma_resample_cost.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("digital-subband-video-1_amd")
    text = ["Cost of chroma resampling in the source and output passes (csrc/k_pixfmt.hip, csrc/k_pixout.hip); written by tools/chroma_cost.py", "",
            "== in: the halving converter against the two calls it replaces"] + in_section(pkg, a.frames, a.rounds) + \
           ["", "== out: the batched decoder writing UYVY from a 4:2:0 stream against NV12"] + out_section(pkg, a.streams, a.rounds)
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))


if __name__ == "__main__":
    main()
