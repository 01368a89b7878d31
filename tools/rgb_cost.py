#!/usr/bin/env python3
"""What RGB costs (dsv1_batch_set_source_rgb, dsv1_decbatch_set_output_rgb, dsv1_rgb_import_clip, dsv1_rgb_export_clip).  1920x1080,
4:2:0, GOP 12, --gops closed GOPs per step.
  1. the passes alone, frames held in HBM: import of RGB24, BGRA and PLANAR_GBR to 4:2:0, export of 4:2:0 to RGB24 / BGRA with both
     upsampling modes, and -- the yardstick -- dsv1_convert_clip and dsv1_export_clip on NV12; the settings ALTERNATE within the run
     (--rounds rounds over all of them after one warm-up round; at most 8 GOPs of frames), each synchronous call timed by the host (stream creation and the
     launch included; the kernels' own time comes from a rocprofv3 --kernel-trace --stats run of this tool with --kernel-only);
     reported as the median and as compulsory bytes (source in + result out) per second, and as a ratio to the NV12 pass of the
     same direction;
  2. the step: one Batch, clip held in HBM (DSV1_CLIP_HELD), fed the planar frames the import gives, then the same pictures as RGB24
     -- the stream hashes must agree -- ms per step each, calls pipelined, the two settings alternating;
  3. dsv1_decbatch_decode per call, --gops streams of one 1080p GOP, device output: packed planar against BGRA (linear), alternating.
Prints one JSON line per figure; writes nothing else.
    python tools/rgb_cost.py [--gops 64] [--steps 4] [--rounds 7] [--kernel-only]"""
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

W, H, GOP, QP, FMT = 1920, 1080, 12, 85, A.SUBSAMP_420


def timed(submit, collect, steps):
    t0 = time.perf_counter()
    submit()
    for _ in range(1, steps):
        submit()
        collect()
    collect()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gops", type=int, default=64)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    pkg = importlib.import_module("digital-subband-video-1_amd")
    L = pkg.lib()
    S, F = a.gops, GOP
    n = min(S, 8) * F                # frames of the passes alone (section 1): enough to fill the device, small enough to make on the host
    planar_fb = A.frame_bytes(W, H, FMT)
    one = A.gen_clip(W, H, A.SUBSAMP_444, 0x7E5, F, style=2).reshape(F, 3, H, W)
    rgb24 = np.ascontiguousarray(np.stack([one[:, 2], one[:, 0], one[:, 1]], axis=-1)).reshape(F, -1)       # R, G, B of moving pictures
    rf = lambda order, up=pkg.CHROMA_LINEAR: pkg.RgbFormat(order, pkg.MATRIX_BT709, 0, up)          # noqa: E731
    nv12 = pkg.PixFormat(pkg.PIX_SEMIPLANAR_UV)
    # 1. the passes alone
    mem = pkg.Batch(pkg.make_encoder_cfg(64, 64, FMT), 1, 1)
    try:
        def dev(nbytes, fill=None):
            if fill is not None:
                return mem.upload(fill)
            p = C.c_void_p(None)
            assert L.dsvg_dev_alloc(mem.ctx, C.byref(p), nbytes) == 0
            return p

        rng = np.random.default_rng(1)
        big = dev(0, rng.integers(0, 256, n * 4 * W * H, dtype=np.uint8))          # source of every import (any bytes are RGB)
        planar = dev(0, rng.integers(0, 256, n * planar_fb, dtype=np.uint8))       # source of every export
        out = dev(n * 4 * W * H)
        runs = [("import RGB24", 3 * W * H + planar_fb, lambda: pkg.rgb_import_clip(big, rf(pkg.RGB_RGB24), W, H, FMT, n=n, out=out)),
                ("import BGRA", 4 * W * H + planar_fb, lambda: pkg.rgb_import_clip(big, rf(pkg.RGB_BGRA), W, H, FMT, n=n, out=out)),
                ("import PLANAR_GBR", 3 * W * H + planar_fb, lambda: pkg.rgb_import_clip(big, rf(pkg.RGB_PLANAR_GBR), W, H, FMT, n=n, out=out)),
                ("import NV12 (dsv1_convert_clip)", 2 * planar_fb, lambda: pkg.convert_clip(big, nv12, W, H, FMT, n=n, out=out)),
                ("export RGB24 linear", 3 * W * H + planar_fb, lambda: pkg.rgb_export_clip(planar, W, H, FMT, rf(pkg.RGB_RGB24), n=n, out=out)),
                ("export RGB24 replicate", 3 * W * H + planar_fb, lambda: pkg.rgb_export_clip(planar, W, H, FMT, rf(pkg.RGB_RGB24, pkg.CHROMA_REPLICATE), n=n, out=out)),
                ("export BGRA linear", 4 * W * H + planar_fb, lambda: pkg.rgb_export_clip(planar, W, H, FMT, rf(pkg.RGB_BGRA), n=n, out=out)),
                ("export BGRA replicate", 4 * W * H + planar_fb, lambda: pkg.rgb_export_clip(planar, W, H, FMT, rf(pkg.RGB_BGRA, pkg.CHROMA_REPLICATE), n=n, out=out)),
                ("export NV12 (dsv1_export_clip)", 2 * planar_fb, lambda: pkg.export_clip(planar, W, H, FMT, nv12, n=n, out=out))]
        ms = {name: [] for name, _, _ in runs}
        for r in range(a.rounds + 1):
            for name, _, fn in runs:
                t0 = time.perf_counter()
                fn()
                if r:                                    # (round 0 warms up)
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        rate = {name: fb * n / statistics.median(ms[name]) / 1e6 for name, fb, _ in runs}
        for name, fb, _ in runs:
            ref = rate["import NV12 (dsv1_convert_clip)" if name.startswith("import") else "export NV12 (dsv1_export_clip)"]
            print(json.dumps(dict(kernel=name, frames=n, host_ms_median=round(statistics.median(ms[name]), 3), host_ms_min=round(min(ms[name]), 3),
                                  compulsory_bytes=fb * n, gb_s=round(rate[name], 1), of_nv12=round(rate[name] / ref, 3))))
    finally:
        mem.close()
    if a.kernel_only:
        return
    # 2. the step, clip held in HBM
    conv = pkg.rgb_import_clip(rgb24, rf(pkg.RGB_RGB24), W, H, FMT)
    cfg = pkg.make_encoder_cfg(W, H, FMT, qp=QP, gop=GOP, rc_mode_cli=1)
    bs, clips, hs, res = {}, {}, {}, {"planar": [], "rgb24": []}
    try:
        for name, src in (("planar", conv), ("rgb24", rgb24)):
            b = bs[name] = pkg.Batch(cfg, S, F)
            if name == "rgb24":
                b.set_source_rgb(rf(pkg.RGB_RGB24))
            clips[name] = b.upload(np.ascontiguousarray(np.broadcast_to(src, (S,) + src.shape)))
            hs[name] = hashlib.sha256()
        for r in range(3):
            for name, b in bs.items():
                def collect(b=b, name=name):
                    for s in b.collect():
                        hs[name].update(s)
                t = timed(lambda b=b, name=name: b.submit(clips[name], on_device=True, held=True), collect, a.steps)
                if r:
                    res[name].append(t)
    finally:
        for b in bs.values():
            b.close()
    assert hs["planar"].hexdigest() == hs["rgb24"].hexdigest(), "the streams differ between planar and RGB24 input"
    for name in res:
        print(json.dumps(dict(step=name, gops=S, ms_per_step=[round(x, 3) for x in res[name]], streams_sha256=hs[name].hexdigest()[:16])))
    print(json.dumps(dict(summary="step", rgb24_minus_planar_ms=round(min(res["rgb24"]) - min(res["planar"]), 3))))
    # 3. the batched decoder, device output
    stream = pkg.encode_clip(conv, W, H, FMT, qp=QP, gop=GOP, rc_mode_cli=1)
    packets = A.split_packets(stream)
    dres = {"planar": [], "bgra": []}
    for r in range(3):
        for name in dres:
            d = pkg.DecBatch(W, H, FMT, S)
            try:
                if name == "bgra":
                    d.set_output_rgb(rf(pkg.RGB_BGRA))
                d.decode([packets[0]] * S, on_device=True)
                calls = []
                for p in packets[1:]:
                    t0 = time.perf_counter()
                    d.decode([p] * S, on_device=True)
                    d.sync()
                    if p[5] & 4:
                        calls.append((time.perf_counter() - t0) * 1e3)
                if r:
                    dres[name].append(statistics.median(calls))
            finally:
                d.close()
    for name in dres:
        print(json.dumps(dict(decode=name, streams=S, ms_per_call_median=[round(x, 3) for x in dres[name]], out_bytes_per_call=S * (planar_fb if name == "planar" else 4 * W * H))))
    print(json.dumps(dict(summary="decode", bgra_minus_planar_ms=round(min(dres["bgra"]) - min(dres["planar"]), 3))))


if __name__ == "__main__":
    main()
