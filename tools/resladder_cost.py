#!/usr/bin/env python3
"""What a resolution ladder (dsv1_resladder_open, Python ResLadder) costs against separate batches fed pre-scaled clips.  Source
1920x1080 4:2:0, GOP 12, --gops closed GOPs per step; geometries 1920x1080 / 1280x720 / 960x540 at one CRF rate each (qp 85); calls
pipelined (submit(i+1); collect(i)).  Forms timed, each over the same --steps calls after one warm-up call:
    resladder-pinned:  ONE ResLadder, the source in pinned host memory (one upload of the 1080p clip per call, two scales on the GPU);
    separate-pinned:   three plain Batches, one per geometry, each fed its PRE-SCALED clip from pinned host memory (three uploads);
    separate-held:     the same with the pre-scaled clips held in HBM (DSV1_CLIP_HELD: no upload at all).
The time the separate forms would need to scale on a CPU is not counted: the comparison favours them.  The separate batches run back to
back (the sum of their times).  Last, the scaler alone: dsv1_scale_clip of the call's clip in HBM to 720p and 540p, timed by the host
around --scale-reps synchronous calls (the kernel's own time comes from a rocprofv3 --kernel-trace run of this tool with --scale-only).
Prints one JSON line per form and a summary; writes nothing else.
    python tools/resladder_cost.py [--gops 64] [--steps 4] [--scale-only]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _cabi as A  # noqa: E402

W, H, FMT, GOP, QP = 1920, 1080, A.SUBSAMP_420, 12, 85
GEOMS = [(1920, 1080), (1280, 720), (960, 540)]


def clip_of(pkg, S, F):
    one = A.gen_clip(W, H, FMT, 0x7E5, F, style=2)
    return np.ascontiguousarray(np.broadcast_to(one, (S, F, one.shape[1])))


def timed(submit, collect, steps):
    submit(0)
    collect()                                   # warm-up call
    t0 = time.perf_counter()
    submit(1)
    for k in range(2, steps + 1):
        submit(k)
        collect()
    collect()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gops", type=int, default=64)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--scale-reps", type=int, default=10)
    ap.add_argument("--scale-only", action="store_true")
    a = ap.parse_args()
    pkg = importlib.import_module("digital-subband-video-1_amd")
    S, F = a.gops, GOP
    src = clip_of(pkg, S, F)
    pix = sum(w * h for w, h in GEOMS) * S * F
    res = {}
    if not a.scale_only:
        cfg = {g: pkg.make_encoder_cfg(g[0], g[1], FMT, qp=QP, gop=GOP, rc_mode_cli=1) for g in GEOMS}
        # resolution ladder, pinned source
        r = pkg.ResLadder(W, H, FMT, [(w, h, [cfg[(w, h)]]) for w, h in GEOMS], S, F, pkg.SCALE_CUBIC)
        try:
            pin = r.pinned(src.shape)
            pin[...] = src
            res["resladder-pinned"] = timed(lambda k: r.submit(pin), r.collect, a.steps)
            up = r.uploads()
        finally:
            r.close()
        scaled = {g: (src if g == (W, H) else pkg.scale_clip(src.reshape(S * F, -1), W, H, FMT, g[0], g[1]).reshape(S, F, -1))
                  for g in GEOMS}
        for form in ("pinned", "held"):
            tot = 0.0
            for g in GEOMS:
                b = pkg.Batch(cfg[g], S, F)
                try:
                    if form == "pinned":
                        x = b.pinned(scaled[g].shape)
                        x[...] = scaled[g]
                        tot += timed(lambda k: b.submit(x), b.collect, a.steps)
                    else:
                        d = b.upload(scaled[g])
                        tot += timed(lambda k: b.submit(d, on_device=True, held=True), b.collect, a.steps)
                finally:
                    b.close()
            res["separate-" + form] = tot
        for k, ms in res.items():
            print(json.dumps(dict(form=k, gops=S, ms_per_call=round(ms, 3), rung_mpix_s=round(pix / ms / 1e3, 1))))
        print(json.dumps(dict(summary=True, resladder_vs_separate_pinned=round(res["separate-pinned"] / res["resladder-pinned"], 3),
                              resladder_vs_separate_held=round(res["separate-held"] / res["resladder-pinned"], 3),
                              resladder_upload_bytes_per_call=up[0] // max(up[1], 1))))
    # the scaler alone, clip in HBM
    L = pkg.lib()
    b = pkg.Batch(pkg.make_encoder_cfg(64, 64, FMT), 1, 1)
    try:
        d = b.upload(src)
        outs = {}
        for g in GEOMS[1:]:
            o = C.c_void_p(None)
            assert L.dsvg_dev_alloc(b.ctx, C.byref(o), S * F * A.frame_bytes(g[0], g[1], FMT)) == 0
            b._dev.append(o)
            outs[g] = o
        for g, o in outs.items():
            pkg.scale_clip(d, W, H, FMT, g[0], g[1], n=S * F, out=o)
            t0 = time.perf_counter()
            for _ in range(a.scale_reps):
                pkg.scale_clip(d, W, H, FMT, g[0], g[1], n=S * F, out=o)
            ms = (time.perf_counter() - t0) * 1e3 / a.scale_reps
            nbytes = S * F * (A.frame_bytes(W, H, FMT) + A.frame_bytes(g[0], g[1], FMT))
            print(json.dumps(dict(scale="%dx%d" % g, frames=S * F, host_ms_per_call=round(ms, 3), compulsory_bytes=nbytes,
                                  host_gb_s=round(nbytes / ms / 1e6, 1))))
    finally:
        b.close()


if __name__ == "__main__":
    main()
