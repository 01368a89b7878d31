#!/usr/bin/env python3
"""What the HDR import costs (dsv1_hdr_import_clip, dsv1_batch_set_source_hdr; csrc/k_hdr.hip).  1920x1080 P010 4:2:0 -> 4:2:0, --frames
pictures held in HBM, PQ / BT.2390 tables of the library.
  1. the calls: dsv1_hdr_import_clip (linear and replicated chroma) against dsv1_convert_clip of the same clip -- what such footage
     costs today, cut to 8 bits -- each synchronous call timed by the host (lane and converter creation, the tables' upload and the
     launch included), the settings ALTERNATING within the run (--rounds rounds after one warm-up round); median and minimum;
  2. the pass alone: one converter and one lane kept, --reps launches enqueued back to back and one wait (a timed window of a quarter of a second for the pass),
     host clock over the lot,
     against -- the yardstick -- a device-to-device copy of the clip's bytes on the same lane; alternating, --rounds rounds after
     one warm-up round.  Reported per picture and as compulsory bytes (source in + result out; the copy: its bytes in and out) per
     second.  (Where the lookup tables live was decided with this section: profiles/hdr_cost.txt has the run that timed the kernel
     with them in LDS against the same kernel reading them from global memory; only the winner is built.)
Prints one JSON line per figure; writes nothing else.
    python tools/hdr_cost.py [--frames 96] [--rounds 7] [--reps 200]"""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _cabi as A  # noqa: E402

W, H, FMT = 1920, 1080, A.SUBSAMP_420


class HdrLayout(C.Structure):
    """dsv1_hdr_layout (csrc/dsvg_pixfmt.h)"""
    _fields_ = [(k, C.c_int) for k in ("w", "h", "shs", "svs", "scw", "sch", "dhs", "dvs", "ocw", "och", "semi", "vshift", "vmask", "rs", "rnd")] + [
        ("off", C.c_size_t * 3), ("pitch", C.c_size_t * 3), ("frame_bytes", C.c_size_t), ("planes_bytes", C.c_size_t), ("out_frame_bytes", C.c_size_t)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    pkg = importlib.import_module("digital-subband-video-1_amd")
    L = pkg.lib()
    n = a.frames
    p010 = pkg.PixFormat(pkg.PIX_SEMIPLANAR_UV, 10, 1)
    sfb = pkg.pix_frame_bytes(p010, W, H, FMT)
    dfb = A.frame_bytes(W, H, FMT)
    tables = pkg.hdr_build(pkg.Hdr(pkg.TRANSFER_PQ, pkg.MATRIX_BT2020, 0, 1, pkg.TONEMAP_BT2390, 1000, 203, pkg.MATRIX_BT709, 0))
    # moving pictures widened to 10 bits, the low bits random: P010 words
    one = A.gen_clip(W, H, FMT, 0x4D12, 8, style=2).astype(np.uint16)
    rng = np.random.default_rng(1)
    words = ((one << 2) | rng.integers(0, 4, one.shape, dtype=np.uint16)) << 6
    cw, ch = A.chroma_dims(W, H, FMT)
    frames = []
    for t in range(8):
        y, u, v = words[t, :W * H], words[t, W * H:W * H + cw * ch], words[t, W * H + cw * ch:]
        frames.append(np.concatenate([y, np.stack([u, v], axis=-1).reshape(-1)]))
    clip = np.ascontiguousarray(np.stack([frames[t % 8] for t in range(n)])).view(np.uint8).reshape(n, sfb)
    mem = pkg.Batch(pkg.make_encoder_cfg(64, 64, FMT), 1, 1)
    lane, conv = C.c_void_p(None), C.c_void_p(None)
    L.dsvg_lane_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.dsvg_lane_stream.restype = C.c_void_p
    for fn in (L.dsvg_lane_stream, L.dsvg_lane_sync, L.dsvg_lane_destroy):
        fn.argtypes = [C.c_void_p]
    L.dsvg_lane_destroy.restype = None
    L.dsvg_lane_copy_dd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.dsv1_hdr_layout_of.argtypes = [C.POINTER(pkg.PixFormat), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(HdrLayout)]
    L.dsvg_pixconv_create_hdr.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(HdrLayout), C.POINTER(pkg.HdrTables), C.c_int]
    L.dsvg_pixconv_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.dsvg_pixconv_destroy.argtypes = [C.c_void_p]
    L.dsvg_pixconv_destroy.restype = None
    try:
        src = mem.upload(clip)
        out = C.c_void_p(None)
        assert L.dsvg_dev_alloc(mem.ctx, C.byref(out), n * sfb) == 0

        def read(nbytes):
            host = np.zeros(nbytes, dtype=np.uint8)
            assert L.dsvg_dev_download(mem.ctx, host.ctypes.data, out, nbytes) == 0
            return host

        # 1. the calls
        runs = [("dsv1_hdr_import_clip linear", sfb + dfb, lambda: pkg.hdr_import_clip(src, p010, W, H, FMT, FMT, tables, pkg.CHROMA_LINEAR, n=n, out=out)),
                ("dsv1_hdr_import_clip replicate", sfb + dfb, lambda: pkg.hdr_import_clip(src, p010, W, H, FMT, FMT, tables, pkg.CHROMA_REPLICATE, n=n, out=out)),
                ("dsv1_convert_clip", sfb + dfb, lambda: pkg.convert_clip(src, p010, W, H, FMT, n=n, out=out))]
        ms = {name: [] for name, _, _ in runs}
        for r in range(a.rounds + 1):
            for name, _, fn in runs:
                t0 = time.perf_counter()
                fn()
                if r:                                    # (round 0 warms up)
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        ref = statistics.median(ms["dsv1_convert_clip"])
        for name, fb, _ in runs:
            med = statistics.median(ms[name])
            print(json.dumps(dict(call=name, frames=n, host_ms_median=round(med, 3), host_ms_min=round(min(ms[name]), 3), us_per_picture=round(med * 1e3 / n, 2),
                                  compulsory_bytes=fb * n, gb_s=round(fb * n / med / 1e6, 1), times_convert_clip=round(med / ref, 3))))
        # 2. the pass alone
        lay = HdrLayout()
        assert L.dsv1_hdr_layout_of(C.byref(p010), W, H, FMT, FMT, C.byref(lay)) == 0 and lay.frame_bytes == sfb and lay.out_frame_bytes == dfb
        assert L.dsvg_lane_create(C.byref(lane), 0) == 0
        assert L.dsvg_pixconv_create_hdr(C.byref(conv), 0, C.byref(lay), C.byref(tables), pkg.CHROMA_LINEAR) == 0
        st = L.dsvg_lane_stream(lane)

        def pass_():
            for _ in range(a.reps):
                assert L.dsvg_pixconv_run(conv, st, src, n, out) == 0
            assert L.dsvg_lane_sync(lane) == 0

        def copy():
            for _ in range(a.reps):
                assert L.dsvg_lane_copy_dd(lane, out, src, n * sfb) == 0
            assert L.dsvg_lane_sync(lane) == 0

        pass_()
        sha = hashlib.sha256(read(n * dfb)).hexdigest()
        alone = [("k_hdr_import", sfb + dfb, pass_), ("device-to-device copy", 2 * sfb, copy)]
        ms = {name: [] for name, _, _ in alone}
        for r in range(a.rounds + 1):
            for name, _, fn in alone:
                t0 = time.perf_counter()
                fn()
                if r:
                    ms[name].append((time.perf_counter() - t0) * 1e3 / a.reps)
        ref = statistics.median(ms["device-to-device copy"])
        for name, fb, _ in alone:
            med = statistics.median(ms[name])
            print(json.dumps(dict(pass_alone=name, frames=n, reps=a.reps, ms_median=round(med, 3), ms_min=round(min(ms[name]), 3), us_per_picture=round(med * 1e3 / n, 2),
                                  compulsory_bytes=fb * n, gb_s=round(fb * n / med / 1e6, 1), times_copy=round(med / ref, 3))))
        print(json.dumps(dict(summary="output", output_sha256=sha[:16])))
    finally:
        if conv.value:
            L.dsvg_lane_sync(lane)
            L.dsvg_pixconv_destroy(conv)
        if lane.value:
            L.dsvg_lane_destroy(lane)
        mem.close()


if __name__ == "__main__":
    main()
