#!/usr/bin/env python3
"""What a source pixel format (dsv1_batch_set_source_format, dsv1_resladder_open_src, dsv1_convert_clip) costs.  1920x1080 4:2:0,
GOP 12, --gops closed GOPs per step (4:2:2 for the packed layouts' kernel figure).
  1. the converter alone, per format: dsv1_convert_clip of --gops x 12 frames held in HBM, timed by the host around --reps synchronous
     calls (stream creation and the launch included; the kernel's own time comes from a rocprofv3 --kernel-trace --stats run of this
     tool with --kernel-only), against its compulsory bytes (source in + planar out);
  2. the step: one Batch, clip held in HBM (DSV1_CLIP_HELD), fed planar frames with no format set, then the same frames as NV12 and
     as P010 -- the stream hashes must agree -- ms per step each, calls pipelined;
  3. the host-fed resolution ladder of tools/resladder_cost.py (1080p / 720p / 540p, pinned source) with a planar and an NV12 source.
Prints one JSON line per figure; writes nothing else.
    python tools/pixfmt_cost.py [--gops 64] [--steps 4] [--reps 10] [--kernel-only]"""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _cabi as A  # noqa: E402
import _pixfmt as PF  # noqa: E402

W, H, GOP, QP = 1920, 1080, 12, 85
GEOMS = [(1920, 1080), (1280, 720), (960, 540)]
KERNEL_FORMATS = [("planar8", PF.pf(), A.SUBSAMP_420), ("nv12", PF.pf(PF.SEMI_UV), A.SUBSAMP_420), ("p010", PF.pf(PF.SEMI_UV, 10, 1), A.SUBSAMP_420),
                  ("yuv420p10le", PF.pf(PF.PLANAR, 10, 0), A.SUBSAMP_420), ("yuyv", PF.pf(PF.YUYV), A.SUBSAMP_422), ("uyvy", PF.pf(PF.UYVY), A.SUBSAMP_422)]


def cpf(pkg, f):
    return pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"])


def raw_clip(one, f, fmt, S):
    """[S, F, raw frame bytes]: the planar 8-bit frames `one` [F, frame_bytes] in format f, the same for every source"""
    vals = one.astype(np.uint32) << (f["depth"] - 8)
    raw = PF.pack(vals, f, W, H, fmt).reshape(one.shape[0], -1)
    return np.ascontiguousarray(np.broadcast_to(raw, (S,) + raw.shape))


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    pkg = importlib.import_module("digital-subband-video-1_amd")
    L = pkg.lib()
    S, F = a.gops, GOP
    # 1. the converter alone
    mem = pkg.Batch(pkg.make_encoder_cfg(64, 64, A.SUBSAMP_420), 1, 1)
    try:
        for name, f, fmt in KERNEL_FORMATS:
            one = A.gen_clip(W, H, fmt, 0x7E5, F, style=2)
            raw = raw_clip(one, f, fmt, S)
            d = mem.upload(raw)
            o = C.c_void_p(None)
            assert L.dsvg_dev_alloc(mem.ctx, C.byref(o), S * F * A.frame_bytes(W, H, fmt)) == 0
            pkg.convert_clip(d, cpf(pkg, f), W, H, fmt, n=S * F, out=o)
            t0 = time.perf_counter()
            for _ in range(a.reps):
                pkg.convert_clip(d, cpf(pkg, f), W, H, fmt, n=S * F, out=o)
            ms = (time.perf_counter() - t0) * 1e3 / a.reps
            nbytes = raw.nbytes + S * F * A.frame_bytes(W, H, fmt)
            print(json.dumps(dict(convert=name, frames=S * F, host_ms_per_call=round(ms, 3), compulsory_bytes=nbytes, host_gb_s=round(nbytes / ms / 1e6, 1))))
            mem.sync()
            L.dsvg_dev_free(mem.ctx, o)
            L.dsvg_dev_free(mem.ctx, mem._dev.pop())
    finally:
        mem.close()
    if a.kernel_only:
        return
    # 2. the step, clip held in HBM
    fmt = A.SUBSAMP_420
    one = A.gen_clip(W, H, fmt, 0x7E5, F, style=2)
    cfg = pkg.make_encoder_cfg(W, H, fmt, qp=QP, gop=GOP, rc_mode_cli=1)
    res, hashes = {}, {}
    for name, f in [("planar", None), ("nv12", PF.pf(PF.SEMI_UV)), ("p010", PF.pf(PF.SEMI_UV, 10, 1))]:
        b = pkg.Batch(cfg, S, F)
        try:
            clip = np.ascontiguousarray(np.broadcast_to(one, (S,) + one.shape)) if f is None else raw_clip(one, f, fmt, S)
            if f is not None:
                b.set_source_format(cpf(pkg, f))
            d = b.upload(clip)
            h = hashlib.sha256()

            def collect():
                for s in b.collect():
                    h.update(s)

            res[name] = timed(lambda k: b.submit(d, on_device=True, held=True), collect, a.steps)
            hashes[name] = h.hexdigest()
        finally:
            b.close()
        print(json.dumps(dict(step=name, gops=S, ms_per_step=round(res[name], 3), streams_sha256=hashes[name][:16])))
    assert hashes["nv12"] == hashes["planar"] and hashes["p010"] == hashes["planar"], "the streams differ between source formats"
    print(json.dumps(dict(summary="step", nv12_minus_planar_ms=round(res["nv12"] - res["planar"], 3), p010_minus_planar_ms=round(res["p010"] - res["planar"], 3))))
    # 3. the host-fed resolution ladder
    rl = {}
    for name, f in [("planar", None), ("nv12", PF.pf(PF.SEMI_UV))]:
        r = pkg.ResLadder(W, H, fmt, [(w, h, [pkg.make_encoder_cfg(w, h, fmt, qp=QP, gop=GOP, rc_mode_cli=1)]) for w, h in GEOMS], S, F, pkg.SCALE_CUBIC,
                          src_format=None if f is None else cpf(pkg, f))
        try:
            clip = np.broadcast_to(one, (S,) + one.shape) if f is None else raw_clip(one, f, fmt, S)
            pin = r.pinned(clip.shape)
            pin[...] = clip
            rl[name] = timed(lambda k: r.submit(pin), r.collect, a.steps)
            up = r.uploads()
        finally:
            r.close()
        print(json.dumps(dict(resladder=name, gops=S, ms_per_call=round(rl[name], 3), upload_bytes_per_call=up[0] // max(up[1], 1))))
    print(json.dumps(dict(summary="resladder", nv12_minus_planar_ms=round(rl["nv12"] - rl["planar"], 3))))


if __name__ == "__main__":
    main()
