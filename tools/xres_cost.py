#!/usr/bin/env python3
"""What measuring resolution-ladder rungs at the source resolution costs (dsv1_resladder_src_quality_enable, k_xres_quality).  Source
1920x1080 4:2:0, GOP 12, --gops closed GOPs per call; geometries 1920x1080 / 1280x720 / 960x540 at one CRF rate each (qp 85); host-fed
calls from pinned memory, pipelined (submit(i+1); collect(i)).  Forms timed, each over the same --steps calls after one warm-up call:
    off:       no measurement;
    rung:      SSE + SSIM of every rung against its own scaled source (sse_enable + ssim_enable);
    source:    SSE + SSIM of every rung upscaled to 1080p against the original source (src_quality_enable, cubic).
The kernel's own time comes from a rocprofv3 --kernel-trace --stats run of this tool with --only source.
Prints one JSON line per form and a summary; writes nothing else.
    python tools/xres_cost.py [--gops 16] [--steps 4] [--only FORM]"""
import argparse
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
FORMS = ("off", "rung", "source")


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
    ap.add_argument("--gops", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--only", choices=FORMS)
    a = ap.parse_args()
    pkg = importlib.import_module("digital-subband-video-1_amd")
    S, F = a.gops, GOP
    one = A.gen_clip(W, H, FMT, 0x7E5, F, style=2)
    src = np.ascontiguousarray(np.broadcast_to(one, (S, F, one.shape[1])))
    cfg = [pkg.make_encoder_cfg(w, h, FMT, qp=QP, gop=GOP, rc_mode_cli=1) for w, h in GEOMS]
    res = {}
    for form in ([a.only] if a.only else FORMS):
        r = pkg.ResLadder(W, H, FMT, [(w, h, [c]) for (w, h), c in zip(GEOMS, cfg)], S, F, pkg.SCALE_CUBIC)
        try:
            if form == "rung":
                r.sse_enable()
                r.ssim_enable()
            elif form == "source":
                r.src_quality_enable(sse=True, ssim=True, filt=pkg.SCALE_CUBIC)
            pin = r.pinned(src.shape)
            pin[...] = src
            res[form] = timed(lambda k: r.submit(pin), r.collect, a.steps)
            if form == "source":
                psnr = r.src_psnr()[:, :, 3].mean(axis=1)
        finally:
            r.close()
        print(json.dumps(dict(form=form, gops=S, pictures_per_call=S * F * len(GEOMS), ms_per_call=round(res[form], 3))))
    if len(res) == len(FORMS):
        upscaled = S * F * len(GEOMS) * W * H * 1.5
        print(json.dumps(dict(summary=True, rung_over_off_ms=round(res["rung"] - res["off"], 3),
                              source_over_off_ms=round(res["source"] - res["off"], 3),
                              source_over_off_pct=round(100 * (res["source"] / res["off"] - 1), 2),
                              source_over_off_us_per_picture=round(1e3 * (res["source"] - res["off"]) / (S * F * len(GEOMS)), 2),
                              measured_samples_per_call=int(upscaled),
                              src_psnr_db_by_geometry=[round(float(psnr[g]), 2) for g in range(len(GEOMS))])))


if __name__ == "__main__":
    main()
