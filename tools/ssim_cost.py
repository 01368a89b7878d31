#!/usr/bin/env python3
"""What the SSIM report (dsv1_batch_ssim_enable, csrc/k_quality.hip k_ssim) costs on the headline shape, next to the SSE report
(tools/sse_cost.py): 1920x1080 4:2:0, GOP 12, --gops closed GOPs per step, the clip held in HBM (DSV1_CLIP_HELD), steps pipelined as
bench.py runs them (submit(i+1); collect(i)).  Loops of --steps steps in the modes off (nothing measured), sse (k_sse), ssim (k_ssim)
and both (one k_ssim pass that makes the SSE too) alternate in ONE process (--rounds rounds); every loop restarts the streams at frame
number 0 (a forced GOP start), so step k of every loop codes the same pictures with the same frame numbers and its packets must be the
same bytes in every mode.  Prints one JSON line per loop and a summary line:
    python tools/ssim_cost.py [--gops 320] [--steps 8] [--rounds 3] [--modes off,sse,ssim,both]
--modes both --rounds 1: only measured loops (a kernel trace of the measurement alone).  Like bench.py, the process first moves to
the host cores the link is best from (shard.pin_single_rank_measured); --no-pin: it stays where it is (under a profiler).  The summary
counts every picture coded with SSIM on (warm-up included): k_ssim's algorithmic bytes are that count x 2 x 1920 x 1080 x 1.5 (source
+ reconstruction of the picture area)."""
import argparse
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

W, H, FMT, GOP, QP = 1920, 1080, A.SUBSAMP_420, 12, 85
MODES = {"off": (False, False), "sse": (True, False), "ssim": (False, True), "both": (True, True)}     # (SSE on, SSIM on)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gops", type=int, default=320)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default="off,sse,ssim,both")
    ap.add_argument("--no-pin", action="store_true")
    ap.add_argument("--distinct", type=int, default=16, help="distinct synthetic GOP clips (bench.py's default and seeds)")
    args = ap.parse_args()
    modes = [m.strip() for m in args.modes.split(",")]
    assert all(m in MODES for m in modes), modes
    placement = None
    if not args.no_pin:
        shard = importlib.import_module("digital-subband-video-1_amd.shard")
        _, node, _ = shard.pin_single_rank_measured(0)        # before anything touches the GPU
        placement = "numa node %s" % node if node is not None else "unpinned"
    pkg = importlib.import_module("digital-subband-video-1_amd")
    if pkg.lib().dsvg_device_count() < 1:
        raise RuntimeError("no HIP device")
    fb = A.frame_bytes(W, H, FMT)
    nd = max(1, min(args.distinct, args.gops))
    distinct = [A.gen_clip(W, H, FMT, 0x10800003 + g, GOP, style=0) for g in range(nd)]
    clip = np.empty((args.gops, GOP, fb), dtype=np.uint8)
    for s in range(args.gops):
        clip[s] = distinct[s % nd]
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, FMT, qp=QP, gop=GOP, rc_mode_cli=1), args.gops, GOP)
    src = b.upload(clip)
    del clip
    pix_step = args.gops * GOP * W * H
    measured = [0]                                          # pictures coded with SSIM on

    def restart():
        # every stream at frame number 0 again, as a GOP start (nothing in flight)
        for s in range(args.gops):
            b.set_fnum(s, 0)
            b.encoder(s).force_metadata = 1

    def loop(mode):
        sse_on, ssim_on = MODES[mode]
        b.sse_enable(sse_on)
        b.ssim_enable(ssim_on)
        restart()
        b.submit(src, on_device=True, held=True)            # fill the pipeline
        measured[0] += args.gops * GOP * (1 + args.steps) * ssim_on
        b.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            b.submit(src, on_device=True, held=True)
            outs = b.collect(copy=False)
        b.sync()
        dt = time.perf_counter() - t0
        h = hashlib.sha256()
        for o in outs:
            h.update(o.view())
        rec = {"mode": mode, "steps": args.steps, "ms_per_step": round(1e3 * dt / args.steps, 3),
               "gpix_s": round(pix_step * args.steps / dt / 1e9, 2), "sha256_last_step": h.hexdigest()}
        if sse_on:
            e = b.sse()
            db = pkg.psnr_db(e, W, H, FMT)
            rec["psnr_db_mean"] = [round(float(v), 3) for v in db.reshape(-1, 4).mean(axis=0)]     # Y, U, V, picture
            rec["sse_sha256"] = hashlib.sha256(e.tobytes()).hexdigest()[:16]
        if ssim_on:
            fx = b.ssim_fx()
            rec["pictures_measured_per_step"] = int(fx.shape[0] * fx.shape[1])
            rec["ssim_mean"] = [round(float(v), 5) for v in pkg.ssim_mean(fx, W, H, FMT).reshape(-1, 4).mean(axis=0)]
        del outs
        b.collect(copy=False)                                # drain
        return rec

    try:
        b.encode(src, on_device=True)                        # warm-up (and the measurement's buffers)
        if modes != ["off"]:
            b.sse_enable(True)                               # (both measurements' buffers)
            b.ssim_enable(True)
            b.encode(src, on_device=True)
            measured[0] += args.gops * GOP
        recs = []
        for _ in range(args.rounds):
            for m in modes:
                r = loop(m)
                print(json.dumps(r), flush=True)
                recs.append(r)
    finally:
        b.close()
    summ = {"shape": "%dx%d 4:2:0 GOP %d, %d GOPs per step, clip held in HBM" % (W, H, GOP, args.gops), "rounds": args.rounds,
            "placement": placement, "pictures_measured_total": measured[0],
            "ssim_algorithmic_bytes_total": measured[0] * 2 * (W * H + 2 * (W // 2) * (H // 2))}
    for m in modes:
        v = [r["gpix_s"] for r in recs if r["mode"] == m]
        summ["gpix_s_" + m] = v
        summ["gpix_s_%s_median" % m] = statistics.median(v)
        summ["ms_per_step_%s_median" % m] = statistics.median([r["ms_per_step"] for r in recs if r["mode"] == m])
    if "off" in modes:
        for m in modes:
            if m != "off":
                summ[m + "_over_off"] = round(summ["gpix_s_%s_median" % m] / summ["gpix_s_off_median"], 4)
    if "sse" in modes and "both" in modes:
        summ["both_minus_sse_ms"] = round(summ["ms_per_step_both_median"] - summ["ms_per_step_sse_median"], 3)
        summ["both_minus_sse_pct_of_sse_step"] = round(100 * summ["both_minus_sse_ms"] / summ["ms_per_step_sse_median"], 2)
        summ["sse_equal_in_sse_and_both"] = len({r["sse_sha256"] for r in recs if "sse_sha256" in r}) == 1
    summ["streams_equal"] = len({r["sha256_last_step"] for r in recs}) == 1
    print(json.dumps({"summary": summ}), flush=True)
    if not summ["streams_equal"]:
        sys.exit("the packets differ between loops")


if __name__ == "__main__":
    main()
