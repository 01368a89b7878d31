#!/usr/bin/env python3
"""What the decoder output scale costs (dsv1_decbatch_set_output_scale; csrc/k_scale.hip k_scale_slots in the output pass of
csrc/dsvg_pipe.hip) against what a caller does without it.  --streams streams of one 1920x1080 4:2:0 GOP, one box, one run, a
decoder of every setting alive and the settings alternating call by call.  Per target (960x540, 480x270), filter (tent, cubic) and
leg (device output; pinned host output):
  scaled       the new path: dsv1_decbatch_decode with the scale in force, output straight at the target size;
  composition  what the same result takes without it: full-size device output, dsv1_resample_clip of that (a synchronous call on a
               lane of its own), with a format dsv1_export_clip of that, and for the host leg the copy of the result to pinned memory;
  full size    plain dsv1_decbatch_decode at the streams' size, the same leg.
With a format on top (NV12, cubic only): scaled + dsv1_decbatch_set_output_format against the composition with dsv1_export_clip.
Every timing is a host clock around work that ends in a device synchronise; per round the median over the GOP's calls, then the
median over the rounds after one warm-up round.  The scaled output and the composition's are compared byte for byte.
Writes profiles/outscale_cost.txt.
    python tools/outscale_cost.py [--streams 64] [--rounds 5] [--gop 8]"""
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

W, H, QP = 1920, 1080, 85
S420 = A.SUBSAMP_420
TARGETS = [(960, 540), (480, 270)]


class Leg:
    """one setting of one leg: a decoder, its buffers and a step(packet) that ends synchronised"""

    def __init__(self, pkg, name, S, target, filt, nv12, composed, host):
        self.pkg, self.L, self.name, self.S, self.host, self.composed = pkg, pkg.lib(), name, S, host, composed
        self.target, self.filt = target, filt
        self.d = pkg.DecBatch(W, H, S420, S)
        self.pf = pkg.PixFormat(pkg.PIX_SEMIPLANAR_UV) if nv12 else None
        dw, dh = target or (W, H)
        self.out_fb = A.frame_bytes(dw, dh, S420)        # (NV12 at 4:2:0 occupies what the planar frame does)
        if not composed:
            if target:
                self.d.set_output_scale(dw, dh, filt)
            if nv12:
                self.d.set_output_format(self.pf)
            assert self.d.frame_bytes == self.out_fb and self.d.out_dims == (dw, dh)
        self.full = self.d.dev_alloc() if composed or not host else None          # the decoder's device output
        self.mid = self._dev(S * self.out_fb) if composed else None               # dsv1_resample_clip's result
        self.fin = self._dev(S * self.out_fb) if composed and nv12 else None      # dsv1_export_clip's result
        self.pin = None
        if host:
            p = C.c_void_p(None)
            assert self.L.dsvg_host_alloc(self.d.ctx, C.byref(p), S * self.out_fb) == 0
            self.pin_p = p
            self.pin = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(S * self.out_fb,)).reshape(S, self.out_fb)

    def _dev(self, nbytes):
        p = C.c_void_p(None)
        assert self.L.dsvg_dev_alloc(self.d.ctx, C.byref(p), nbytes) == 0
        return p

    def step(self, packet):
        pk = [packet] * self.S
        if not self.composed:
            if self.host:
                self.d.decode(pk, out=self.pin)          # (synchronises)
            else:
                self.d.decode(pk, out=self.full, on_device=True)
                self.d.sync()
            return
        self.d.decode(pk, out=self.full, on_device=True)
        self.d.sync()
        if not packet[5] & 4:
            return
        last = self.pkg.resample_clip(self.full, W, H, S420, self.target[0], self.target[1], self.filt, n=self.S, out=self.mid)
        if self.fin is not None:
            last = self.pkg.export_clip(self.mid, self.target[0], self.target[1], S420, self.pf, n=self.S, out=self.fin)
        if self.host:
            assert self.L.dsvg_dev_download(self.d.ctx, self.pin.ctypes.data, last, self.pin.nbytes) == 0

    def result(self):
        """the last call's frames as the caller has them"""
        if self.host:
            return self.pin.copy()
        last = self.full if not self.composed else (self.fin if self.fin is not None else self.mid)
        out = np.zeros((self.S, self.out_fb), dtype=np.uint8)
        self.d.sync()
        assert self.L.dsvg_dev_download(self.d.ctx, out.ctypes.data, last, out.nbytes) == 0
        return out

    def close(self):
        if self.pin is not None:
            self.pin = None
            self.L.dsvg_host_free(self.d.ctx, self.pin_p)
        self.d.close()


def section(pkg, packets, S, rounds, host, target, filt, nv12):
    what = "%dx%d %s%s" % (target + ("cubic" if filt == pkg.SCALE_CUBIC else "tent", " + NV12" if nv12 else ""))
    specs = [("scaled: " + what, target, False), ("composition: " + what, target, True), ("full size%s" % (" NV12" if nv12 else ""), None, False)]
    ms = {name: [] for name, _, _ in specs}
    legs = []
    try:
        for name, tg, composed in specs:
            legs.append(Leg(pkg, name, S, tg, filt, nv12, composed, host))
        for r in range(rounds + 1):
            calls = {name: [] for name in ms}
            for p in packets:
                for leg in legs:
                    t0 = time.perf_counter()
                    leg.step(p)
                    if p[5] & 4:
                        calls[leg.name].append((time.perf_counter() - t0) * 1e3)
            if r:                                        # (round 0 warms up)
                for name in calls:
                    ms[name].append(statistics.median(calls[name]))
        same = np.array_equal(legs[0].result(), legs[1].result())
        assert same, "the scaled output and the composition's differ: " + what
    finally:
        for leg in legs:
            leg.close()
    ref = statistics.median(ms[specs[1][0]])
    lines = []
    for (name, tg, _), leg in zip(specs, legs):
        med = statistics.median(ms[name])
        lines.append("%-44s %10.3f %10.3f %16d %14.3f" % (name, med, min(ms[name]), S * leg.out_fb, med / ref))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gop", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outscale_cost.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("digital-subband-video-1_amd")
    if pkg.lib().dsvg_device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    clip = A.gen_clip(W, H, S420, 0x05CA1E, a.gop, style=2)
    packets = A.split_packets(pkg.encode_clip(clip, W, H, S420, qp=QP, gop=a.gop, rc_mode_cli=1))
    text = ["Cost of the decoder output scale (csrc/k_scale.hip k_scale_slots in the output pass); written by tools/outscale_cost.py", "",
            "dsv1_decbatch_decode of %d streams of one %dx%d 4:2:0 GOP (%d pictures, -qp%d); each call timed on the host up to its synchronise;" % (
                a.streams, W, H, a.gop, QP),
            "a decoder of every setting alive, alternating call by call; per round the median over the GOP's calls, %d rounds after one" % a.rounds,
            "warm-up.  composition: full-size device output, then dsv1_resample_clip, then dsv1_export_clip where a format is set, then (host",
            "leg) the copy of the result to pinned memory -- what a caller does without the output scale.  The scaled output and the",
            "composition's were compared byte for byte in every section."]
    for host in (False, True):
        text += ["", "== %s output" % ("pinned host" if host else "device"),
                 "%-44s %10s %10s %16s %14s" % ("setting", "median ms", "min ms", "out bytes / call", "x composition")]
        for target in TARGETS:
            for filt, nv12 in ((pkg.SCALE_TENT, False), (pkg.SCALE_CUBIC, False), (pkg.SCALE_CUBIC, True)):
                text += section(pkg, packets, a.streams, a.rounds, host, target, filt, nv12)
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))


if __name__ == "__main__":
    main()
